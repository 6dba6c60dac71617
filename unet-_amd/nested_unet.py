"""Drop-in for the reference's ``NestedUNet`` (src/models/unetpp.py:28-135) in inference use.

Same constructor keywords, the nn.Module surface the frame loops touch (``.to``, ``.eval``,
``.load_state_dict``, ``__call__``) and the same results; the work is done by hand-written HIP
kernels behind the C ABI of include/unetpp.h.  PyTorch tensors are only I/O buffers (``data_ptr()``)
and the source of the current HIP stream — no torch op runs on the hot path.  This file is the model: engine, weights, the
forward family, status, profile and debug hooks; the post-processing methods are the mixin of postproc.py.

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
from .postproc import PostProcessing


class NestedUNet(PostProcessing):
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
        x: float32 [B,3,H,W] (any values up to +-65504: status() says when one was clamped) or uint8 [B,H,W,3] BGR frames at
        model resolution.
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

    def predict_proba(self, x, output: int = 0):
        """softmax(model(x), dim=1) as float32 [B,C,H,W] on the device (one fused pass); output=k (1..3): of
        deep-supervision output k, from a pruned pass (see forward)."""
        return self._run(x, False, False, False, True, output=output)[4]

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

    def profile_plan(self):
        """[(launch name, grid, tiles, ksplit, rows per wave)] of the last forward (profiling on), in profile_read()'s
        order: the plan of every persistent launch (tiles counts split-K shares); zeros for the other launches."""
        lib = _lib.load()
        out = []
        for i in range(lib.unetpp_profile_count(self._handle)):
            plan = (ctypes.c_int * 4)()
            rc = lib.unetpp_profile_plan(self._handle, i, plan)
            if rc != 0:
                raise RuntimeError(self._err(rc))
            out.append((lib.unetpp_profile_name(self._handle, i).decode(), *[int(v) for v in plan]))
        return out

    def debug_keep_intermediates(self, on: bool = True):
        """Materialise x0_4 and run the head unfused (needed before debug_activation('x0_4')).  In 'exact' conv0_4.conv1 then
        also runs in the plain fused-upsample kernel instead of conv3x3_ws_uprows_kernel: same layer, another
        plan, logits within 5e-6.  That layer only: conv1_3.conv1, which runs in the same kernel as two 32-channel tiles, keeps
        the plan its engine was created with (UNETPP_UPROWS picks the levels; its weights are packed for that kernel)."""
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
