"""Drop-in for the reference's ``NestedUNet`` (src/models/unetpp.py:28-135) in inference use.

Same constructor keywords, the nn.Module surface the frame loops touch (``.to``, ``.eval``,
``.load_state_dict``, ``__call__``) and the same results; the work is done by hand-written HIP
kernels behind the C ABI of include/unetpp.h.  PyTorch tensors are only I/O buffers (``data_ptr()``)
and the source of the current HIP stream — no torch op runs on the hot path.

    model = NestedUNet(num_classes=3, deep_supervision=True, pretrained_encoder=False).to(device)   # infer_two_stage_burr.py:214
    model.load_state_dict(checkpoint['model'], strict=True); model.eval()                           # :215-217
    outputs = model(img_tensor)                                                                      # :294-297
    pred = model.segment(img_tensor)       # fused replacement of :294-300 (uint8 class-index mask, on device)
    out, out1, out2, out3 = model.forward_deep_supervision(img_tensor)   # the list of unetpp.py:121-133, one pass
    pred1 = model.segment(img_tensor, output=1)   # pruned UNet++: stops after x1_3 and uses the ds1_3 head
    cable = model.filter_components(pred, 1, rule="largest", min_area=50)   # src/utils/geometry_enhanced.py:140, on device
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _lib, packing


class NestedUNet:
    _ARCH = _lib.ARCH_NESTED
    _SIZE_MULTIPLE = 16
    def __init__(self, num_classes: int, input_channels: int = 3, deep_supervision: bool = True,
                 pretrained_encoder: bool = False, *, precision: str = "exact", max_batch: int = 16,
                 max_hw=(512, 512), micro_batch: int = 0, streams: int = 1, check_range: bool = False) -> None:
        if pretrained_encoder:
            # unetpp.py:52-65 swaps in a torchvision ResNet50 and downloads ImageNet weights; no
            # north-star caller uses it (infer_two_stage_burr.py:214) and there is no network here.
            raise NotImplementedError("pretrained_encoder=True is unsupported by the MI355X engine")
        if input_channels != 3:
            raise NotImplementedError("input_channels must be 3")
        if precision not in _lib.PRECISIONS:
            raise ValueError("precision must be 'exact', 'exact8' or 'fast'")
        self.num_classes = int(num_classes)
        self.input_channels = int(input_channels)
        self.deep_supervision = bool(deep_supervision)
        self.training = False
        self.precision = precision
        self._max_batch = int(max_batch)
        self._max_hw = (int(max_hw[0]), int(max_hw[1]))
        self._micro_batch = int(micro_batch)
        self._streams = int(streams)
        self._keep_all = False
        self._check_range = bool(check_range)      # debug aid: synchronise and raise after a forward that left the fp16 range
        self._device_index: Optional[int] = None
        self._handle = None
        self._blob: Optional[np.ndarray] = None      # canonical weights (host copy, re-uploaded if the engine is rebuilt)
        self._ds_blob: Optional[np.ndarray] = None   # deep-supervision heads (host copy, uploaded on the first ds call)
        self._ds_uploaded = False                    # ... to the current engine
        self._state_dict = None
        self._cc_workspaces = {}                     # components(): scratch per (B, H, W, max_components)
        self._morph_programs = {}                    # morphology programs in their ctypes form, per parameter set

    # ------------------------------------------------------------------ nn.Module surface
    def to(self, device):
        import torch
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"device '{dev}': the MI355X engine runs on HIP devices only (no CPU fallback); "
                               "use the reference model for --device cpu")
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        if self._device_index is not None and idx != self._device_index:
            self._destroy()
        self._device_index = idx
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else f"cuda:{device}")

    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("inference-only engine: train() is unsupported")
        return self.eval()

    def load_state_dict(self, state_dict, strict: bool = True):
        state_dict = packing.unwrap_checkpoint(state_dict)
        missing, unexpected = packing.check_state_dict(state_dict, self.num_classes, self.input_channels,
                                                       self.deep_supervision, strict)
        if missing:
            raise RuntimeError("Missing key(s) in state_dict: " + ", ".join(missing))
        self._blob = packing.build_blob(state_dict, self.num_classes, self.input_channels)
        self._ds_blob = packing.build_ds_blob(state_dict, self.num_classes) if self.deep_supervision else None
        self._ds_uploaded = False
        self._state_dict = {k: packing._np(v).copy() for k, v in state_dict.items()}
        if self._handle is not None:
            self._upload()
        return missing, unexpected

    def state_dict(self):
        if self._state_dict is None:
            raise RuntimeError("no weights loaded")
        return dict(self._state_dict)

    def __call__(self, x):
        return self.forward(x)

    # ------------------------------------------------------------------ engine management
    def _err(self, rc: int) -> str:
        lib = _lib.load()
        msg = lib.unetpp_last_error(self._handle)
        return f"unetpp error {rc}: {msg.decode() if msg else ''}"

    def _destroy(self):
        if self._handle is not None:
            _lib.load().unetpp_destroy(self._handle)
            self._handle = None
        self._ds_uploaded = False

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def _ensure_engine(self, b: int, h: int, w: int):
        if self._device_index is None:
            raise RuntimeError("call .to('cuda:N') first: the MI355X engine has no CPU path")
        grow = (self._handle is None or b > self._max_batch or h > self._max_hw[0] or w > self._max_hw[1])
        if not grow:
            return
        self._destroy()
        self._max_batch = max(self._max_batch, b)
        self._max_hw = (max(self._max_hw[0], h), max(self._max_hw[1], w))
        lib = _lib.load()
        cfg = _lib.Config(self.num_classes, self.input_channels, self._max_batch, self._max_hw[0], self._max_hw[1],
                          _lib.PRECISIONS[self.precision], self._device_index,
                          self._micro_batch, self._streams, self._ARCH)
        handle = ctypes.c_void_p()
        rc = lib.unetpp_create(ctypes.byref(cfg), ctypes.byref(handle))
        if rc != 0:
            msg = lib.unetpp_last_error(None)
            raise RuntimeError(f"unetpp_create failed ({rc}): {msg.decode() if msg else ''}")
        self._handle = handle
        if self._keep_all:
            lib.unetpp_debug_keep_intermediates(self._handle, 1)
        if self._blob is not None:
            self._upload()

    def _upload(self):
        lib = _lib.load()
        self._ds_uploaded = False                    # the engine drops its ds heads with new main weights
        rc = lib.unetpp_load_weights(self._handle, self._blob.ctypes.data_as(ctypes.c_void_p), self._blob.nbytes)
        if rc != 0:
            raise RuntimeError(self._err(rc))

    def _upload_ds(self):
        """The deep-supervision heads, on the first ds call of an engine (also after a rebuild)."""
        if self._ds_blob is None:      # weights from load_weights_from_device_blob: the broadcast blob has no ds heads
            raise RuntimeError("no deep-supervision heads loaded: load_state_dict() a checkpoint with ds3_1 / ds2_2 / ds1_3 "
                               "(sharding.load_replicated broadcasts the main blob only)")
        if self._ds_uploaded:
            return
        rc = _lib.load().unetpp_load_ds_heads(self._handle, self._ds_blob.ctypes.data_as(ctypes.c_void_p), self._ds_blob.nbytes)
        if rc != 0:
            raise RuntimeError(self._err(rc))
        self._ds_uploaded = True

    def _check_output(self, output):
        """output = k selects the reference's deep-supervision list entry [out, out1, out2, out3][k]."""
        if self._ARCH != _lib.ARCH_NESTED:
            raise NotImplementedError(f"output={output!r}: deep-supervision outputs exist for NestedUNet only")
        if isinstance(output, bool) or not isinstance(output, (int, np.integer)) or not 0 <= int(output) <= 3:
            raise ValueError(f"output must be 0 (out), 1 (out1, ds1_3), 2 (out2, ds2_2) or 3 (out3, ds3_1), got {output!r}")
        if output and not self.deep_supervision:
            raise ValueError(f"output={output}: the model was built with deep_supervision=False and has no ds heads")
        return int(output)

    def _check_and_build_blob(self, state_dict):
        """strict key check + canonical blob of this architecture (rank 0 of sharding.load_replicated)."""
        state_dict = packing.unwrap_checkpoint(state_dict)
        packing.check_state_dict(state_dict, self.num_classes, self.input_channels, self.deep_supervision, strict=True)
        return packing.build_blob(state_dict, self.num_classes, self.input_channels)

    def load_weights_from_device_blob(self, blob_tensor):
        """After an RCCL broadcast: `blob_tensor` is a uint8 CUDA tensor holding the canonical blob."""
        import torch
        self._ensure_engine(1, self._SIZE_MULTIPLE, self._SIZE_MULTIPLE)
        rc = _lib.load().unetpp_load_weights_device(self._handle, ctypes.c_void_p(blob_tensor.data_ptr()),
                                                    blob_tensor.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RuntimeError(self._err(rc))
        self._blob = blob_tensor.cpu().numpy()
        self._ds_blob = None                         # the broadcast carries no ds heads: output != 0 is refused
        self._ds_uploaded = False

    # ------------------------------------------------------------------ the hot path
    def _prepare(self, x):
        """Checks the input, builds (or grows) the engine; returns (x contiguous, input format, b, h, w)."""
        import torch
        if self.training:
            raise RuntimeError("engine is inference-only")
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("input must be a CUDA (HIP) tensor on the engine's device")
        if self._blob is None:
            raise RuntimeError("load_state_dict() must be called before forward")
        if x.dtype == torch.float32:
            if x.dim() != 4 or x.shape[1] != self.input_channels:
                raise RuntimeError(f"expected input [B,{self.input_channels},H,W], got {tuple(x.shape)}")
            b, _, h, w = x.shape
            fmt = _lib.IN_F32_NCHW
        elif x.dtype == torch.uint8:
            if x.dim() != 4 or x.shape[3] != 3:
                raise RuntimeError(f"expected uint8 frames [B,H,W,3] (BGR), got {tuple(x.shape)}")
            b, h, w, _ = x.shape
            fmt = _lib.IN_U8_NHWC_BGR
        else:
            raise RuntimeError(f"unsupported input dtype {x.dtype}")
        if h % self._SIZE_MULTIPLE or w % self._SIZE_MULTIPLE:
            # same failure the reference hits inside torch.cat (unetpp.py:112-116) for such sizes
            raise RuntimeError(f"Sizes of tensors must match: H={h}, W={w} must be multiples of {self._SIZE_MULTIPLE}")
        if self._device_index is None:
            self.to(x.device)
        if x.device.index != self._device_index:
            raise RuntimeError(f"input on {x.device}, engine on cuda:{self._device_index}")
        x = x.contiguous()
        self._ensure_engine(b, h, w)
        return x, fmt, b, h, w

    def _run(self, x, want_logits: bool, want_mask: bool, want_class_masks: bool, want_probs: bool = False,
             rule: str = "argmax", params=(0.0, 0.0, 0.0, 0.0), output: int = 0):
        import torch
        output = self._check_output(output) if output != 0 else 0
        x, fmt, b, h, w = self._prepare(x)
        dev = x.device
        logits = torch.empty((b, self.num_classes, h, w), dtype=torch.float32, device=dev) if want_logits else None
        mask = torch.empty((b, h, w), dtype=torch.uint8, device=dev) if want_mask else None
        cable = torch.empty((b, h, w), dtype=torch.uint8, device=dev) if want_class_masks else None
        tape = torch.empty((b, h, w), dtype=torch.uint8, device=dev) if want_class_masks else None
        probs = torch.empty((b, self.num_classes, h, w), dtype=torch.float32, device=dev) if want_probs else None
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if rule not in _lib.RULES:
            raise ValueError(f"rule must be one of {sorted(_lib.RULES)}")
        outs = _lib.Outputs(p(logits), p(probs), p(mask), p(cable), p(tape), _lib.RULES[rule], *[float(v) for v in params])
        if output == 0:
            rc = _lib.load().unetpp_forward_ex(self._handle, p(x), fmt, b, h, w, ctypes.byref(outs), stream)
        else:      # pruned: only output k is requested, the engine stops after its node
            self._upload_ds()
            lst = (ctypes.POINTER(_lib.Outputs) * 4)()
            lst[output] = ctypes.pointer(outs)
            rc = _lib.load().unetpp_forward_ds(self._handle, p(x), fmt, b, h, w, lst, stream)
        if rc != 0:
            raise RuntimeError(self._err(rc))
        if self._check_range:
            self.raise_on_range_error()
        if want_probs:
            return logits, mask, cable, tape, probs
        return logits, mask, cable, tape

    # ------------------------------------------------------------------ value-range status
    def status(self, clear: bool = False) -> int:
        """Sticky range flags of the engine (include/unetpp.h: UNETPP_STATUS_OVERFLOW = 1, UNETPP_STATUS_NAN = 2):
        set when an activation or input value did not fit the fp16 planes the engine stores activations in — the
        fp32 reference (unetpp.py:23-26) has no such limit, so a non-zero status means the results may differ from
        it.  Synchronises the device."""
        if self._handle is None:
            return 0
        flags = ctypes.c_uint32(0)
        rc = _lib.load().unetpp_status(self._handle, ctypes.byref(flags), 1 if clear else 0)
        if rc != 0:
            raise RuntimeError(self._err(rc))
        return int(flags.value)

    def raise_on_range_error(self):
        """RuntimeError if any forward since the last check left the fp16 range (clears the flags)."""
        flags = self.status(clear=True)
        if flags:
            what = [n for bit, n in ((_lib.STATUS_OVERFLOW, "activation/input beyond +-65504 clamped"),
                                     (_lib.STATUS_NAN, "NaN encountered")) if flags & bit]
            raise RuntimeError("unetpp: value range of the fp16 activation planes exceeded (" + "; ".join(what) +
                               "): results differ from the fp32 reference")

    def forward(self, x, output: int = 0):
        """NestedUNet.forward in eval mode (unetpp.py:93-135): float32 [B,3,H,W] -> float32 logits [B,C,H,W].
        output=k (1..3) returns entry k of the deep-supervision list [out, out1, out2, out3] instead (unetpp.py:121-133),
        from a pass that stops after that entry's node (pruned UNet++)."""
        return self._run(x, True, False, False, output=output)[0]

    def forward_deep_supervision(self, x):
        """[out, out1, out2, out3] of the reference's deep-supervision forward (unetpp.py:121-133, BatchNorm in eval
        mode) as float32 CUDA tensors [B,C,H,W], from one engine pass."""
        import torch
        self._check_output(1)
        x, fmt, b, h, w = self._prepare(x)
        self._upload_ds()
        outs = [torch.empty((b, self.num_classes, h, w), dtype=torch.float32, device=x.device) for _ in range(4)]
        recs = [_lib.Outputs(ctypes.c_void_p(t.data_ptr()), None, None, None, None, 0, 0.0, 0.0, 0.0, 0.0) for t in outs]
        lst = (ctypes.POINTER(_lib.Outputs) * 4)(*[ctypes.pointer(r) for r in recs])
        rc = _lib.load().unetpp_forward_ds(self._handle, ctypes.c_void_p(x.data_ptr()), fmt, b, h, w, lst,
                                           ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
        if rc != 0:
            raise RuntimeError(self._err(rc))
        if self._check_range:
            self.raise_on_range_error()
        return outs

    def segment(self, x, return_logits: bool = False, return_class_masks: bool = False, output: int = 0):
        """Fused model call + softmax/argmax/uint8 (+ class masks) of infer_two_stage_burr.py:294-304.
        x: float32 [B,3,H,W] in [0,1] or uint8 [B,H,W,3] BGR frames at model resolution.
        output=k (1..3): the same on deep-supervision output k, from a pruned pass (see forward)."""
        logits, mask, cable, tape = self._run(x, return_logits, True, return_class_masks, output=output)
        out = (mask,)
        if return_class_masks:
            out += (cable, tape)
        if return_logits:
            out += (logits,)
        return out[0] if len(out) == 1 else out

    def segment_thresholded(self, x, rule: str = "thresholded_argmax", t_cable: float = 0.45, t_tape: float = 0.50,
                            bg_margin: float = 0.15, ct_margin: float = 0.10, return_probs: bool = False, output: int = 0):
        """The thresholded frame loops' tail on the device: probs = softmax_np(outputs) then
        `thresholded_argmax` (infer_video_3class_best.py:56-83, infer_video_strict.py:36-63),
        `strict_bg_check` (infer_video_fixed.py:35-83: bg_margin is the background-probability ceiling) or
        `exclusive` (infer_video_robust.py:70-99).  Returns (mask_cable, mask_tape[, probs[B,C,H,W]]) on device.
        output=k (1..3): on deep-supervision output k, from a pruned pass (see forward)."""
        r = self._run(x, False, False, True, return_probs, rule, (t_cable, t_tape, bg_margin, ct_margin), output=output)
        return (r[2], r[3], r[4]) if return_probs else (r[2], r[3])

    def mask_stats(self, mask):
        """Device-side reductions of a uint8 class-index mask [B,H,W] (e.g. from segment()):
        returns (counts int64 [B,C], widths float32 [B,C,H]) where counts[b,c] = np.sum(mask[b]==c)
        (infer_two_stage_burr.py:333-334) and widths[b,c,y] = xs.max()-xs.min()+1 over the columns of class c
        in row y, 0 for empty rows (_compute_width_per_row, src/utils/geometry_enhanced.py:45-74, before its
        optional smoothing).  Only B*C*(2H+1) integers cross to the caller instead of the mask."""
        import torch
        if not (isinstance(mask, torch.Tensor) and mask.is_cuda and mask.dtype == torch.uint8 and mask.dim() == 3):
            raise RuntimeError("mask must be a uint8 CUDA tensor [B,H,W]")
        if self._handle is None:
            raise RuntimeError("engine not initialised: run a forward first")
        mask = mask.contiguous()
        b, h, w = mask.shape
        c = self.num_classes
        counts = torch.empty((b, c), dtype=torch.int32, device=mask.device)
        rmin = torch.empty((b, c, h), dtype=torch.int32, device=mask.device)
        rmax = torch.empty((b, c, h), dtype=torch.int32, device=mask.device)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = _lib.load().unetpp_mask_stats(self._handle, p(mask), b, h, w, p(counts), p(rmin), p(rmax),
                                           ctypes.c_void_p(torch.cuda.current_stream(mask.device).cuda_stream))
        if rc != 0:
            raise RuntimeError(self._err(rc))
        widths = torch.where(rmax >= 0, (rmax - rmin + 1), torch.zeros_like(rmax)).to(torch.float32)
        return counts.to(torch.int64), widths

    # ------------------------------------------------------------------ connected components
    def _components(self, mask, match_class, connectivity, max_components, want_stats: bool):
        import torch
        if not (isinstance(mask, torch.Tensor) and mask.is_cuda and mask.dtype == torch.uint8 and mask.dim() == 3):
            raise RuntimeError("mask must be a uint8 CUDA tensor [B,H,W]")
        if connectivity not in (4, 8):
            raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
        k = int(max_components)
        if k < 2:
            raise ValueError(f"max_components must be at least 2 (background + one component), got {max_components!r}")
        if self._device_index is None:
            self.to(mask.device)
        if mask.device.index != self._device_index:
            raise RuntimeError(f"mask on {mask.device}, engine on cuda:{self._device_index}")
        self._ensure_engine(1, self._SIZE_MULTIPLE, self._SIZE_MULTIPLE)
        mask = mask.contiguous()
        b, h, w = mask.shape
        lib = _lib.load()
        key = (b, h, w, k)
        cache = self._cc_workspaces
        ws = cache.get(key)
        if ws is None or ws.device != mask.device:
            nbytes = int(lib.unetpp_components_workspace_bytes(b, h, w, k))
            if nbytes == 0:
                raise RuntimeError(f"components: unsupported shape {tuple(mask.shape)}")
            ws = cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=mask.device)
        dev = mask.device
        labels = torch.empty((b, h, w), dtype=torch.int32, device=dev)
        num = torch.empty((b,), dtype=torch.int32, device=dev)
        stats = torch.empty((b, k, 5), dtype=torch.int32, device=dev) if want_stats else None
        sums = torch.empty((b, k, 2), dtype=torch.int64, device=dev) if want_stats else None   # uint64 bits; values < 2^63
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        rc = lib.unetpp_components(self._handle, p(mask), b, h, w, int(match_class), int(connectivity), k, p(labels), p(num),
                                   p(stats), p(sums), p(ws), stream)
        if rc != 0:
            raise RuntimeError(self._err(rc))
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
        if isinstance(out_value, bool) or not isinstance(out_value, (int, np.integer)) or not 1 <= int(out_value) <= 255:
            raise ValueError(f"out_value must be an integer in 1..255, got {out_value!r}")
        import torch
        labels, num, stats, sums, ws, stream = self._components(mask, match_class, connectivity, max_components, True)
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
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = _lib.load().unetpp_components_filter(self._handle, p(labels), p(num), p(stats), p(sums), b, h, w, k,
                                                  _lib.CC_RULES[rule], ctypes.byref(params), int(out_value), p(out), p(ws), stream)
        if rc != 0:
            raise RuntimeError(self._err(rc))
        if check:
            n = num.cpu().tolist()
            for i, v in enumerate(n):
                if v > k:
                    raise RuntimeError(f"filter_components: frame {i} has num = {v} labels (background included), more than "
                                       f"max_components = {k}: raise max_components")
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
        for m in (mask0,) + (() if mask1 is None else (mask1,)):
            if not (isinstance(m, torch.Tensor) and m.is_cuda and m.dtype == torch.uint8 and m.dim() == 3):
                raise RuntimeError("mask must be a uint8 CUDA tensor [B,H,W]")
        if mask1 is not None and (mask1.shape != mask0.shape or mask1.device != mask0.device):
            raise RuntimeError(f"mask1 {tuple(mask1.shape)} on {mask1.device} does not match mask0 {tuple(mask0.shape)} on {mask0.device}")
        if self._device_index is None:
            self.to(mask0.device)
        if mask0.device.index != self._device_index:
            raise RuntimeError(f"mask on {mask0.device}, engine on cuda:{self._device_index}")
        self._ensure_engine(1, self._SIZE_MULTIPLE, self._SIZE_MULTIPLE)
        mask0 = mask0.contiguous()
        mask1 = None if mask1 is None else mask1.contiguous()
        b, h, w = mask0.shape
        _, c_el, n_el, c_st, n_st, result = compiled
        out = torch.empty((b, h, w), dtype=torch.uint8, device=mask0.device)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        rc = _lib.load().unetpp_morphology(self._handle, p(mask0), int(match0), p(mask1), int(match1), b, h, w, c_el, n_el, c_st, n_st,
                                           result, out_value, p(out), ctypes.c_void_p(torch.cuda.current_stream(mask0.device).cuda_stream))
        if rc != 0:
            raise (ValueError if rc == -2 else RuntimeError)(self._err(rc))
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
            for i, v in enumerate(num.cpu().tolist()):
                if v > k:
                    raise RuntimeError(f"filter_components: frame {i} has num = {v} labels (background included), more than "
                                       f"max_components = {k}: raise max_components")
        return num_holes, hole_area

    # ------------------------------------------------------------------ measurements (unet_amd/geometry.py is the NumPy form)
    @staticmethod
    def _stream(t):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)

    @staticmethod
    def _raise_overflow(over, k, what):
        """`over` bool [B] on the device (one read-back, synchronises): the frames whose labelling overflowed."""
        bad = over.nonzero().flatten().cpu().tolist()
        if bad:
            raise RuntimeError(f"{what}: frame {bad[0]} has more than max_components - 1 = {k - 1} components in one of its "
                               f"labellings: raise max_components")

    def row_widths(self, mask0, match0: int = -1, mask1=None, match1: int = -1):
        """_compute_width_per_row(smooth=False) (src/utils/geometry_enhanced.py:61-67) of two binary planes of uint8
        CUDA masks [B,H,W] in one launch: plane 0 = (mask0 == match0), plane 1 = (mask1 == match1) (match < 0: != 0;
        mask1 may be mask0 itself, or None for an empty plane 1).  Returns (widths float32 [B,2,H] = last - first + 1
        over the foreground columns of a row, 0 for an empty row; area int64 [B,2] = foreground pixels)."""
        import torch
        mask0 = self._edge_input(mask0, "mask0")
        if mask1 is not None:
            same = mask1 is mask0
            mask1 = mask0 if same else self._edge_input(mask1, "mask1")
            if mask1.shape != mask0.shape:
                raise RuntimeError(f"mask1 {tuple(mask1.shape)} does not match mask0 {tuple(mask0.shape)}")
        b, h, w = mask0.shape
        widths = torch.empty((b, 2, h), dtype=torch.float32, device=mask0.device)
        area = torch.empty((b, 2), dtype=torch.int32, device=mask0.device)            # uint32 bits
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        rc = _lib.load().unetpp_row_widths(self._handle, p(mask0), int(match0), p(mask1), int(match1), b, h, w, p(widths), p(area),
                                           self._stream(mask0))
        if rc != 0:
            self._raise(rc)
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
        if not (isinstance(widths, torch.Tensor) and widths.is_cuda and widths.dtype == torch.float32 and widths.dim() == 3 and
                widths.shape[1] == 2):
            raise RuntimeError("widths must be a float32 CUDA tensor [B,2,H]")
        if self._device_index is None:
            self.to(widths.device)
        if widths.device.index != self._device_index:
            raise RuntimeError(f"widths on {widths.device}, engine on cuda:{self._device_index}")
        self._ensure_engine(1, self._SIZE_MULTIPLE, self._SIZE_MULTIPLE)
        widths = widths.contiguous()
        b, _, h = widths.shape
        if h > ge.MAX_ROWS:
            raise ValueError(f"width_profile: {h} rows, at most {ge.MAX_ROWS}")
        dev = widths.device
        smoothed = torch.empty_like(widths)
        valid = torch.empty((b, h), dtype=torch.uint8, device=dev)
        delta = torch.empty((b, h), dtype=torch.float32, device=dev) if want_delta else None
        out = torch.empty((b, 3), dtype=torch.int32, device=dev)                      # {float dc_px, dt_px; int32 valid_rows}
        p = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
        rc = _lib.load().unetpp_width_profile(self._handle, p(widths), b, h, t.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(t),
                                              int(min_valid_rows), p(smoothed), p(valid), p(delta), p(out), self._stream(widths))
        if rc != 0:
            self._raise(rc)
        med = out[:, :2].view(torch.float32)
        return smoothed, valid, delta, med[:, 0], med[:, 1], out[:, 2]

    def components_summary(self, num, stats, min_area: int = 0):
        """The reductions analyze_defects makes of a statistics table (geometry_enhanced.py:291-294, :302-309) from `num`
        int32 [B] and `stats` int32 [B,K,5] of components() (stats may be None): int64 [B,4] on the device =
        (max(0, num - 1); labels 1..min(num, K)-1 with area >= min_area; the sum of those areas; the largest area)."""
        import torch
        if not (isinstance(num, torch.Tensor) and num.is_cuda and num.dtype == torch.int32 and num.dim() == 1):
            raise RuntimeError("num must be an int32 CUDA tensor [B]")
        b = num.shape[0]
        if stats is None:
            k = 2
        else:
            if not (isinstance(stats, torch.Tensor) and stats.is_cuda and stats.dtype == torch.int32 and stats.dim() == 3 and
                    stats.shape[0] == b and stats.shape[2] == 5):
                raise RuntimeError("stats must be an int32 CUDA tensor [B,K,5]")
            stats, k = stats.contiguous(), stats.shape[1]
        if self._device_index is None:
            self.to(num.device)
        self._ensure_engine(1, self._SIZE_MULTIPLE, self._SIZE_MULTIPLE)
        num = num.contiguous()
        out = torch.empty((b, 4), dtype=torch.int64, device=num.device)
        p = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
        rc = _lib.load().unetpp_components_summary(self._handle, p(num), p(stats), b, k, int(min_area), p(out), self._stream(num))
        if rc != 0:
            self._raise(rc)
        return out

    def _filter_largest(self, pred, match_class, min_area, k):
        """filter_components(rule='largest', check=False) that also hands back `num`: (uint8 [B,H,W], int32 [B])."""
        import torch
        labels, num, stats, sums, ws, stream = self._components(pred, match_class, 8, k, True)
        b, h, w = labels.shape
        params = _lib.CcRule(float(min_area), 50.0, 300.0, 0.3, 1.6, 0.3, float(w))
        out = torch.empty((b, h, w), dtype=torch.uint8, device=labels.device)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = _lib.load().unetpp_components_filter(self._handle, p(labels), p(num), p(stats), p(sums), b, h, w, k,
                                                  _lib.CC_RULES["largest"], ctypes.byref(params), 1, p(out), p(ws), stream)
        if rc != 0:
            self._raise(rc)
        return out, num

    def _profile_of_largest(self, pred, cls0, cls1, min_area, kernel_size, taps, min_valid_rows, k, want_delta):
        from . import geometry as ge
        t = ge.resolve_taps(kernel_size, taps)
        pred = self._edge_input(pred, "pred")
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
        pred = self._edge_input(pred, "pred")
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
        pred = self._edge_input(pred, "pred")
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
    def _edge_input(self, img, what="gray", channels=None):
        """A contiguous uint8 CUDA image batch on the engine's device, with the engine made ready."""
        import torch
        dims = 3 if channels is None else 4
        if not (isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == torch.uint8 and img.dim() == dims and
                (channels is None or img.shape[-1] == channels)):
            shape = "[B,H,W]" if channels is None else f"[B,H,W,{channels}]"
            raise RuntimeError(f"{what} must be a uint8 CUDA tensor {shape}")
        if self._device_index is None:
            self.to(img.device)
        if img.device.index != self._device_index:
            raise RuntimeError(f"{what} on {img.device}, engine on cuda:{self._device_index}")
        self._ensure_engine(1, self._SIZE_MULTIPLE, self._SIZE_MULTIPLE)
        return img.contiguous()

    def _raise(self, rc):
        raise (ValueError if rc == -2 else RuntimeError)(self._err(rc))

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
        frames = self._edge_input(frames, "frames", 3)
        b, h, w, _ = frames.shape
        out = torch.empty((b, h, w), dtype=torch.uint8, device=frames.device)
        rc = _lib.load().unetpp_gray_u8(self._handle, ctypes.c_void_p(frames.data_ptr()), b, h, w, ctypes.c_void_p(out.data_ptr()),
                                        ctypes.c_void_p(torch.cuda.current_stream(frames.device).cuda_stream))
        if rc != 0:
            self._raise(rc)
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
        gray = self._edge_input(gray)
        b, h, w = gray.shape
        out = torch.empty_like(gray)
        rc = _lib.load().unetpp_gaussian_blur_u8(self._handle, ctypes.c_void_p(gray.data_ptr()), b, h, w, self._c_taps(t), len(t),
                                                 ctypes.c_void_p(out.data_ptr()),
                                                 ctypes.c_void_p(torch.cuda.current_stream(gray.device).cuda_stream))
        if rc != 0:
            self._raise(rc)
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
        gray = self._edge_input(gray)
        b, h, w = gray.shape
        lib = _lib.load()
        key = ("canny", b, h, w)
        ws = self._cc_workspaces.get(key)
        if ws is None or ws.device != gray.device:
            nbytes = int(lib.unetpp_canny_workspace_bytes(b, h, w))
            if nbytes == 0:
                raise RuntimeError(f"canny: unsupported shape {tuple(gray.shape)}")
            ws = self._cc_workspaces[key] = torch.empty(nbytes, dtype=torch.uint8, device=gray.device)
        out = torch.empty_like(gray)
        rc = lib.unetpp_canny_u8(self._handle, ctypes.c_void_p(gray.data_ptr()), b, h, w, self._c_taps(t), 0 if t is None else len(t),
                                 low, high, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                                 ctypes.c_void_p(torch.cuda.current_stream(gray.device).cuda_stream))
        if rc != 0:
            self._raise(rc)
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
        labels, num, stats, _, ws, stream = self._components(mask, match_class, connectivity, max_components, True)
        b, h, w = labels.shape
        k = int(max_components)
        params = _lib.CcBoxRule(*box)
        out = torch.empty((b, h, w), dtype=torch.uint8, device=labels.device)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = _lib.load().unetpp_components_filter_box(self._handle, p(labels), p(num), p(stats), b, h, w, k, ctypes.byref(params),
                                                      out_value, p(out), p(ws), stream)
        if rc != 0:
            self._raise(rc)
        if check:
            for i, v in enumerate(num.cpu().tolist()):
                if v > k:
                    raise RuntimeError(f"filter_components: frame {i} has num = {v} labels (background included), more than "
                                       f"max_components = {k}: raise max_components")
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
        if hasattr(gray, "shape") and hasattr(mask_cable, "shape") and tuple(gray.shape) != tuple(mask_cable.shape):
            raise RuntimeError(f"gray {tuple(gray.shape)} and mask_cable {tuple(mask_cable.shape)} differ in shape")
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
        if hasattr(gray, "shape") and hasattr(mask_cable, "shape") and tuple(gray.shape) != tuple(mask_cable.shape):
            raise RuntimeError(f"gray {tuple(gray.shape)} and mask_cable {tuple(mask_cable.shape)} differ in shape")
        gray = self._edge_input(gray)
        band = self._morph_launch(program, mask_cable, match_class, None, -1, 1)
        b, h, w = gray.shape
        hot = torch.empty_like(gray)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = _lib.load().unetpp_laplacian_band_u8(self._handle, p(gray), p(band), b, h, w, thr, p(hot),
                                                  ctypes.c_void_p(torch.cuda.current_stream(gray.device).cuda_stream))
        if rc != 0:
            self._raise(rc)
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
        gray = self._edge_input(gray)
        if canny_edges is None:
            canny_edges = out = self.canny(gray, canny_low, canny_high, blur=blur)       # ORed in place: the image is ours
        else:
            self._same_shape(gray, canny_edges, "canny_edges")
            canny_edges = self._edge_input(canny_edges, "canny_edges")
            out = torch.empty_like(gray)
        b, h, w = gray.shape
        lib = _lib.load()
        key = ("edges_union", b)
        ws = self._cc_workspaces.get(key)
        if ws is None or ws.device != gray.device:
            ws = self._cc_workspaces[key] = torch.empty(int(lib.unetpp_edges_union_workspace_bytes(b)), dtype=torch.uint8, device=gray.device)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = lib.unetpp_edges_union_u8(self._handle, p(gray), p(canny_edges), b, h, w, sthr, lthr, p(ws), p(out),
                                       ctypes.c_void_p(torch.cuda.current_stream(gray.device).cuda_stream))
        if rc != 0:
            self._raise(rc)
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
        gray, band = self._edge_input(gray), self._edge_input(band, "band")
        b, h, w = gray.shape
        hot = torch.empty_like(gray)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = _lib.load().unetpp_dog_band_u8(self._handle, p(gray), p(band), b, h, w, self._c_taps(t1), len(t1), self._c_taps(t2), len(t2),
                                            thr, p(hot), ctypes.c_void_p(torch.cuda.current_stream(gray.device).cuda_stream))
        if rc != 0:
            self._raise(rc)
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
        mask = self._edge_input(mask, "mask")
        b, h, w = mask.shape
        counts = torch.empty((b,), dtype=torch.int32, device=mask.device)      # uint32 bits; H * W <= 2^30
        rc = _lib.load().unetpp_count_nonzero_u8(self._handle, ctypes.c_void_p(mask.data_ptr()), b, h, w, ctypes.c_void_p(counts.data_ptr()),
                                                 ctypes.c_void_p(torch.cuda.current_stream(mask.device).cuda_stream))
        if rc != 0:
            self._raise(rc)
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
        import torch
        if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8 and
                (frames.dim() == 3 or (frames.dim() == 4 and frames.shape[-1] == 3))):
            raise RuntimeError(f"{what} must be a uint8 CUDA tensor [B,H,W,3] or [B,H,W]")
        return self._edge_input(frames, what, 3 if frames.dim() == 4 else None), (3 if frames.dim() == 4 else 1)

    def _enhance(self, frames, cin, cout, mode, threshold, clip_limit, tile_grid, table, tables, want_luts=False, want_decisions=False):
        """unetpp_enhance_u8: one memset and three launches on the current stream, nothing read back."""
        import torch
        from . import enhance as en
        b, h, w = frames.shape[:3]
        tx, ty = en.grid_of(tile_grid)
        en.check_limits(h, w, (tx, ty), None if tables is None else tables[0])
        if b > 65535:
            raise ValueError(f"batch {b}: at most 65535")
        lib = _lib.load()
        key = ("enhance", b, h, w, tx, ty)
        ws = self._cc_workspaces.get(key)
        if ws is None or ws.device != frames.device:
            nbytes = int(lib.unetpp_enhance_workspace_bytes(b, h, w, tx, ty))
            if nbytes == 0:
                raise RuntimeError(f"enhance: unsupported shape {tuple(frames.shape)} with a {tx}x{ty} grid")
            ws = self._cc_workspaces[key] = torch.empty(nbytes, dtype=torch.uint8, device=frames.device)
        dev = frames.device
        out = torch.empty((b, h, w, 3) if cout == 3 else (b, h, w), dtype=torch.uint8, device=dev)
        luts = torch.empty((b, ty * tx, 256), dtype=torch.uint8, device=dev) if want_luts else None
        dec = torch.empty((b,), dtype=torch.uint8, device=dev) if want_decisions else None
        ct, keep = self._c_tables(tables)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        rc = lib.unetpp_enhance_u8(self._handle, p(frames), b, h, w, cin, cout, mode, float(threshold), float(clip_limit), tx, ty,
                                   None if table is None else table.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                   None if ct is None else ctypes.byref(ct), p(out), p(luts), p(dec), p(ws), self._stream(frames))
        del keep
        if rc != 0:
            self._raise(rc)
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
        rc = _lib.load().unetpp_gray_decision(self._handle, ctypes.c_void_p(frames.data_ptr()), b, h, w, float(threshold),
                                              ctypes.c_void_p(dec.data_ptr()), ctypes.c_void_p(sums.data_ptr()), self._stream(frames))
        if rc != 0:
            self._raise(rc)
        return (dec != 0, sums) if return_sums else dec != 0

    def clahe(self, gray, clip_limit: float = 2.0, tile_grid=(8, 8), return_luts: bool = False):
        """cv2.createCLAHE(clip_limit, tile_grid).apply(gray) for uint8 CUDA images [B,H,W] as OpenCV's CLAHE_Impl::apply
        computes it (enhance.clahe_np; cv2's own result is unpinned).  tile_grid = (tilesX, tilesY) or one number, 1..16
        per side, H > tilesY, W > tilesX.  return_luts: also the per-tile tables uint8 [B, tilesY * tilesX, 256]."""
        gray = self._edge_input(gray)
        out, luts, _ = self._enhance(gray, 1, 1, _lib.ENHANCE_ALWAYS, 0.0, clip_limit, tile_grid, None, None, want_luts=return_luts)
        return (out, luts) if return_luts else out

    def bilateral_filter(self, gray, d: int = 5, sigma_color: float = 75.0, sigma_space: float = 75.0, tables=None):
        """cv2.bilateralFilter(gray, d, sigma_color, sigma_space) for uint8 CUDA images [B,H,W] as OpenCV's scalar 8-bit
        loop computes it (enhance.bilateral_np; cv2's own result is unpinned), radius <= 4 (d <= 9), H, W > radius.
        tables: enhance.bilateral_tables' tuple instead, e.g. with cv2's own weights or tap order."""
        import torch
        from . import enhance as en
        tables = en.check_tables(en.bilateral_tables(d, sigma_color, sigma_space) if tables is None else tables)
        gray = self._edge_input(gray)
        b, h, w = gray.shape
        en.check_limits(h, w, None, tables[0])
        out = torch.empty_like(gray)
        ct, keep = self._c_tables(tables)
        rc = _lib.load().unetpp_bilateral_u8(self._handle, ctypes.c_void_p(gray.data_ptr()), b, h, w, ctypes.byref(ct),
                                             ctypes.c_void_p(out.data_ptr()), self._stream(gray))
        del keep
        if rc != 0:
            self._raise(rc)
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
        if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4):
            raise RuntimeError("frames must be a uint8 CUDA tensor [B,H,W,C]")
        H, W = int(size_hw[0]), int(size_hw[1])
        self._ensure_engine(1, self._SIZE_MULTIPLE, self._SIZE_MULTIPLE)
        frames = frames.contiguous()
        b, h, w, c = frames.shape
        out = torch.empty((b, H, W, c), dtype=torch.uint8, device=frames.device)
        rc = _lib.load().unetpp_resize_linear_u8(self._handle, ctypes.c_void_p(frames.data_ptr()), b, h, w, c,
                                                 ctypes.c_void_p(out.data_ptr()), H, W,
                                                 ctypes.c_void_p(torch.cuda.current_stream(frames.device).cuda_stream))
        if rc != 0:
            raise RuntimeError(self._err(rc))
        return out

    def resize_masks(self, pred, frame_size_wh, match_class: int = -1, roi=None):
        """infer_two_stage_burr.py:303-314 on the device for a uint8 CUDA mask [B,H,W]: optional
        `(pred == match_class)`, cv2.resize(..., (width, height), INTER_NEAREST), zeros outside
        roi = (x1, y1, x2, y2).  Returns uint8 [B,height,width]."""
        import torch
        if not (isinstance(pred, torch.Tensor) and pred.is_cuda and pred.dtype == torch.uint8 and pred.dim() == 3):
            raise RuntimeError("pred must be a uint8 CUDA tensor [B,H,W]")
        fw, fh = int(frame_size_wh[0]), int(frame_size_wh[1])
        x1, y1, x2, y2 = (0, 0, fw, fh) if roi is None else (int(v) for v in roi)
        self._ensure_engine(1, self._SIZE_MULTIPLE, self._SIZE_MULTIPLE)
        pred = pred.contiguous()
        b, h, w = pred.shape
        out = torch.empty((b, fh, fw), dtype=torch.uint8, device=pred.device)
        rc = _lib.load().unetpp_resize_nearest_roi_u8(self._handle, ctypes.c_void_p(pred.data_ptr()), b, h, w,
                                                      int(match_class), ctypes.c_void_p(out.data_ptr()), fh, fw,
                                                      x1, y1, x2, y2,
                                                      ctypes.c_void_p(torch.cuda.current_stream(pred.device).cuda_stream))
        if rc != 0:
            raise RuntimeError(self._err(rc))
        return out

    def predict_proba(self, x, output: int = 0):
        """softmax(model(x), dim=1) as float32 [B,C,H,W] on the device (one fused pass); output=k (1..3): of
        deep-supervision output k, from a pruned pass (see forward)."""
        return self._run(x, False, False, False, True, output=output)[4]

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
        frames = self._edge_input(frames, "frames", 3)
        b, h, w, _ = frames.shape
        plan = tl.tile_plan(h, w, patch_size, stride)
        self._check_plan(plan, h, w, patch_size)
        tl.check_padding(h, w, int(patch_size))
        ys, xs, pys, pxs = self._c_origins(plan)
        out = torch.empty((b * plan.n_patches, t, t, 3), dtype=torch.uint8, device=frames.device)
        rc = _lib.load().unetpp_tile_gather_u8(self._handle, ctypes.c_void_p(frames.data_ptr()), b, h, w, pys, len(ys), pxs, len(xs),
                                               int(patch_size), t, tl.CHANNEL_ORDERS[channel_order], ctypes.c_void_p(out.data_ptr()),
                                               self._stream(frames))
        if rc != 0:
            self._raise(rc)
        return out

    def _check_maps(self, maps):
        import torch
        if not (isinstance(maps, torch.Tensor) and maps.is_cuda and maps.dtype == torch.float32 and maps.dim() == 4 and
                maps.shape[2] == maps.shape[3]):
            raise RuntimeError("maps must be a float32 CUDA tensor [N,C,T,T]")
        if self._device_index is None:
            self.to(maps.device)
        if maps.device.index != self._device_index:
            raise RuntimeError(f"maps on {maps.device}, engine on cuda:{self._device_index}")
        self._ensure_engine(1, self._SIZE_MULTIPLE, self._SIZE_MULTIPLE)
        return maps.contiguous()

    def tile_gate(self, maps, gate_thr, gate_class: int = 1):
        """The window gate of OptimizedSlidingWindowInference.predict (tools/inference_binary_optimized.py:91-98) for
        probability maps float32 CUDA [N,C,T,T]: (include uint8 [N] = score >= gate_thr, scores float32 [N] = the maximum
        of class gate_class over the patch), one launch, nothing read back."""
        import torch
        maps = self._check_maps(maps)
        n, c, t, _ = maps.shape
        if not 0 <= int(gate_class) < c:
            raise ValueError(f"gate_class {gate_class} not in [0,{c})")
        scores = torch.empty((n,), dtype=torch.float32, device=maps.device)
        include = torch.empty((n,), dtype=torch.uint8, device=maps.device)
        rc = _lib.load().unetpp_tile_gate_f32(self._handle, ctypes.c_void_p(maps.data_ptr()), n, c, t, int(gate_class), float(gate_thr),
                                              ctypes.c_void_p(scores.data_ptr()), ctypes.c_void_p(include.data_ptr()), self._stream(maps))
        if rc != 0:
            self._raise(rc)
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
        maps = self._check_maps(maps)
        n, c, t, _ = maps.shape
        if n % plan.n_patches:
            raise RuntimeError(f"maps hold {n} patches, the plan for {h}x{w} has {plan.n_patches} per frame")
        if c > tl.MAX_CLASSES:
            raise ValueError(f"unsupported: {c} classes, at most {tl.MAX_CLASSES}")
        b = n // plan.n_patches
        if include is not None:
            if not (isinstance(include, torch.Tensor) and include.is_cuda and include.dtype == torch.uint8 and tuple(include.shape) == (n,)):
                raise RuntimeError(f"include must be a uint8 CUDA tensor [{n}]")
            include = include.contiguous()
        ys, xs, pys, pxs = self._c_origins(plan)
        mask = torch.empty((b, h, w), dtype=torch.uint8, device=maps.device)
        output = torch.empty((b, h, w, c), dtype=torch.float32, device=maps.device) if return_output else None
        p = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
        rc = _lib.load().unetpp_tile_blend_f32(self._handle, p(maps), b, c, t, pys, len(ys), pxs, len(xs), int(patch_size), p(include),
                                               h, w, p(mask), p(output), self._stream(maps))
        if rc != 0:
            self._raise(rc)
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
        frames = self._edge_input(frames, "frames", 3)
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
            dst = ctypes.c_void_p(maps[k:k + nb].data_ptr())
            outs = _lib.Outputs(dst if blend == "logits" else None, dst if blend == "probs" else None, None, None, None,
                                _lib.RULES["argmax"], 0.0, 0.0, 0.0, 0.0)
            rc = _lib.load().unetpp_forward_ex(self._handle, ctypes.c_void_p(x.data_ptr()), fmt, nb, t, t, ctypes.byref(outs), self._stream(x))
            if rc != 0:
                raise RuntimeError(self._err(rc))
        if self._check_range:
            self.raise_on_range_error()
        include = None if gate_thr is None else self.tile_gate(maps, gate_thr, gate_class)[0]
        return self.blend_tiles(maps, (h, w), patch_size, stride, include, return_output)

    # ------------------------------------------------------------------ measurement / debug hooks
    def workspace_bytes(self) -> int:
        return int(_lib.load().unetpp_workspace_bytes(self._handle)) if self._handle else 0

    def profile(self, on: bool = True):
        _lib.load().unetpp_profile_enable(self._handle, 1 if on else 0)

    def profile_read(self):
        """[(launch name, ms, algorithmic flops, min HBM bytes)] of the last forward (profiling on)."""
        lib = _lib.load()
        n = lib.unetpp_profile_count(self._handle)
        ms = (ctypes.c_float * max(n, 1))()
        got = lib.unetpp_profile_read(self._handle, ms, n)
        if got < 0:
            raise RuntimeError(self._err(got))
        out = []
        for i in range(got):
            fl, by = ctypes.c_double(), ctypes.c_double()
            lib.unetpp_profile_work(self._handle, i, ctypes.byref(fl), ctypes.byref(by))
            out.append((lib.unetpp_profile_name(self._handle, i).decode(), float(ms[i]), fl.value, by.value))
        return out

    def debug_keep_intermediates(self, on: bool = True):
        """Materialise x0_4 and run the head unfused (needed before debug_activation('x0_4'))."""
        self._keep_all = bool(on)                    # also applied to an engine that is (re)built later
        if self._handle is not None:
            _lib.load().unetpp_debug_keep_intermediates(self._handle, 1 if on else 0)

    def _node_shape(self, name: str):
        lvl = int(name[1])
        return (32, 64, 128, 256, 512)[lvl], lvl

    def debug_activation(self, name: str, b: int, h: int, w: int) -> np.ndarray:
        """float32 [b,C,h',w'] copy of an intermediate node ('x0_0'..'x4_0','x3_1','x2_2','x1_3','x0_4')."""
        c, lvl = self._node_shape(name)
        out = np.empty((b, c, h >> lvl, w >> lvl), dtype=np.float32)
        n = _lib.load().unetpp_debug_read(self._handle, name.encode(), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.size)
        if n < 0:
            raise RuntimeError(self._err(int(n)))
        if n != out.size:
            raise RuntimeError(f"debug_read returned {n} floats, expected {out.size}")
        return out


class SimpleUNet(NestedUNet):
    """Drop-in for the reference's ``SimpleUNet`` (src/models/simple_unet.py:20-128), the
    plain 4-level U-Net of infer_video_simple.py:67: same constructor keywords (num_classes=7, num_channels=3),
    same state_dict keys (enc1.0 ... final), logits from ``model(x)``; ``predict_proba`` replaces the
    ``torch.softmax(output, dim=1)`` of infer_video_simple.py:96.  H and W must be multiples of 8."""
    _ARCH = _lib.ARCH_SIMPLE
    _SIZE_MULTIPLE = 8

    def __init__(self, num_classes: int = 7, num_channels: int = 3, *, precision: str = "exact", max_batch: int = 16,
                 max_hw=(256, 256), micro_batch: int = 0, streams: int = 1, check_range: bool = False) -> None:
        super().__init__(num_classes, num_channels, False, False, precision=precision, max_batch=max_batch,
                         max_hw=max_hw, micro_batch=micro_batch, streams=streams, check_range=check_range)
        self.num_channels = int(num_channels)

    def load_state_dict(self, state_dict, strict: bool = True):
        state_dict = packing.unwrap_checkpoint(state_dict)
        missing, unexpected = packing.check_simple_state_dict(state_dict, self.num_classes, self.num_channels, strict)
        if missing:
            raise RuntimeError("Missing key(s) in state_dict: " + ", ".join(missing))
        self._blob = packing.build_simple_blob(state_dict, self.num_classes, self.num_channels)
        self._state_dict = {k: packing._np(v).copy() for k, v in state_dict.items()}
        if self._handle is not None:
            self._upload()
        return missing, unexpected

    def _check_and_build_blob(self, state_dict):
        state_dict = packing.unwrap_checkpoint(state_dict)
        packing.check_simple_state_dict(state_dict, self.num_classes, self.num_channels, strict=True)
        return packing.build_simple_blob(state_dict, self.num_classes, self.num_channels)

    def _node_shape(self, name: str):
        lvl = int(name[3]) - 1                      # 'enc1'..'enc4', 'dec1'..'dec3'
        return (64, 128, 256, 512)[lvl], lvl
