"""FrameStream: a double-buffered driver for the frame loops, so that the copies to and from the device run under the compute.

    fs = FrameStream([model_a, model_b], lambda m, frames: frame_loop.process_frames_two_stage(m, frames, check=False),
                     outputs=("result", "counts"))
    for out in fs.map(batches):              # batches: uint8 NumPy arrays [B,H,W,3]; out: {"result": ..., "counts": ...} NumPy
        ...

Every model is a slot with a stream of its own, a pinned input buffer, a device input buffer and pinned output buffers.  submit()
copies the batch into the slot's pinned buffer and queues, on the slot's stream, the upload, fn(model, device_frames), the
downloads of the tensors fn returned and an event; result() waits for that event alone.  With two slots the upload and download of
one batch overlap the kernels of the other; one slot gives the same results in sequence.  An engine has one workspace, so a model
serves one slot: two slots need two loaded models.  Pure Python on torch streams: no kernel of its own, no captured graph, no queue
setting.  fn should not synchronise (for the loops with an overflow check, pass check=False); it still works if it does, without
the overlap."""
from __future__ import annotations

import collections

import numpy as np

Ticket = collections.namedtuple("Ticket", "slot serial")


class _Slot:
    def __init__(self, torch, model, device):
        self.model = model
        self.stream = torch.cuda.Stream(device=device)
        self.event = torch.cuda.Event()
        self.pinned_in = self.dev_in = None
        self.pinned_out = {}
        self.serial = 0                       # the submission the buffers belong to
        self.pending = False                  # submitted and not yet waited for
        self.error = self.layout = None


def _members(out):
    """(kind, [(key, value)]) of what fn returned: a tensor, a dict, a namedtuple or a tuple / list."""
    if isinstance(out, dict):
        return "dict", list(out.items())
    if isinstance(out, tuple) and hasattr(out, "_fields"):
        return "dict", list(zip(out._fields, out))
    if isinstance(out, (tuple, list)):
        return "tuple", list(enumerate(out))
    return "single", [(0, out)]


class FrameStream:
    def __init__(self, models, fn, *, outputs=None):
        """models: one loaded model or a sequence of them, all on one device, each given once.  fn(model, device_frames) runs a
        loop and returns a tensor, a tuple, a dict or a named tuple; its CUDA tensors are downloaded -- all of them, or those
        `outputs` names (field names or keys; positions for a tuple) -- and every other member is handed through as it is."""
        import torch
        models = list(models) if isinstance(models, (list, tuple)) else [models]
        if not models:
            raise ValueError("FrameStream needs at least one model")
        if len({id(m) for m in models}) != len(models):
            raise ValueError("the same model was given twice: an engine has one workspace, so every slot needs a model of its own")
        if not callable(fn):
            raise TypeError("fn must be callable: fn(model, device_frames)")
        devices = {getattr(m, "_device_index", None) for m in models}
        if None in devices:
            raise ValueError("every model must be on a device: model.to('cuda:0') first")
        if len(devices) != 1:
            raise ValueError(f"the models are on {len(devices)} devices (cuda:{sorted(devices)}), a FrameStream drives one")
        if outputs is not None:
            outputs = tuple(outputs)
            if not outputs or any(not isinstance(o, (str, int)) or isinstance(o, bool) for o in outputs):
                raise ValueError("outputs must name at least one member of fn's result: field names, keys or positions")
        self._torch, self._fn, self._outputs = torch, fn, outputs
        self.device = torch.device("cuda", devices.pop())
        self._slots = [_Slot(torch, m, self.device) for m in models]
        self._next = 0

    @property
    def n_slots(self):
        return len(self._slots)

    def submit(self, frames_np):
        """Queue one batch (a NumPy array whose first axis is the batch; a shorter last batch is fine) on the next slot and return
        its ticket.  Waits first if that slot's previous batch is still running: a slot is reused only after its event."""
        torch = self._torch
        frames = np.ascontiguousarray(frames_np)
        if frames.ndim < 1 or frames.shape[0] < 1:
            raise ValueError(f"a batch needs at least one frame, got an array of shape {frames.shape}")
        index = self._next % len(self._slots)
        slot = self._slots[index]
        self._next += 1
        if slot.pending:
            slot.event.synchronize()
        slot.serial, slot.pending, slot.error, slot.layout = slot.serial + 1, True, None, None
        dtype = torch.from_numpy(frames[:0]).dtype
        b = frames.shape[0]
        with torch.cuda.stream(slot.stream):
            if (slot.pinned_in is None or slot.pinned_in.dtype != dtype or tuple(slot.pinned_in.shape[1:]) != frames.shape[1:] or
                    slot.pinned_in.shape[0] < b):
                slot.pinned_in = torch.empty(frames.shape, dtype=dtype, pin_memory=True)
                slot.dev_in = torch.empty(frames.shape, dtype=dtype, device=self.device)
            slot.pinned_in[:b].numpy()[...] = frames
            dev = slot.dev_in[:b]
            dev.copy_(slot.pinned_in[:b], non_blocking=True)
            try:
                kind, members = _members(self._fn(slot.model, dev))
                if self._outputs is not None:
                    missing = [o for o in self._outputs if o not in dict(members)]
                    if missing:
                        raise KeyError(f"fn's result has no member {missing[0]!r}; it has {[k for k, _ in members]}")
                layout = []
                for key, value in members:
                    if not (isinstance(value, torch.Tensor) and value.device.type == self.device.type):
                        if self._outputs is None or key in self._outputs:
                            layout.append((key, None, value))
                        continue
                    if self._outputs is not None and key not in self._outputs:
                        continue
                    value = value.contiguous()
                    host = slot.pinned_out.get(key)
                    if host is None or host.dtype != value.dtype or host.numel() < value.numel():
                        host = slot.pinned_out[key] = torch.empty(max(value.numel(), 1), dtype=value.dtype, pin_memory=True)
                    view = host[:value.numel()].view(value.shape)
                    view.copy_(value, non_blocking=True)
                    layout.append((key, view, None))
                slot.layout = (kind, layout)
            except Exception as exc:                  # surfaces from result(); the slot stays usable
                slot.error = exc
            slot.event.record(slot.stream)
        return Ticket(index, slot.serial)

    def result(self, ticket):
        """Wait for the ticket's batch alone and return fn's result with NumPy arrays in place of its tensors (a dict for a dict
        or a named tuple).  The arrays are views of the slot's pinned buffers: valid until that slot takes another batch.
        An exception fn raised for this batch is raised here."""
        slot = self._slots[ticket.slot]
        if ticket.serial != slot.serial:
            raise RuntimeError("this ticket's slot has taken another batch since: its results are gone")
        slot.event.synchronize()
        slot.pending = False
        if slot.error is not None:
            raise slot.error
        kind, layout = slot.layout
        values = [(key, passed if view is None else view.numpy()) for key, view, passed in layout]
        if kind == "dict":
            return dict(values)
        if kind == "tuple":
            return tuple(v for _, v in values)
        return values[0][1]

    def map(self, batches):
        """Yield result() of every batch of the iterable, in submission order, with as many batches in flight as there are
        slots.  What it yields is valid until the next item is asked for."""
        waiting = collections.deque()
        for batch in batches:
            if len(waiting) == len(self._slots):
                yield self.result(waiting.popleft())
            waiting.append(self.submit(batch))
        while waiting:
            yield self.result(waiting.popleft())

    def synchronize(self):
        """Wait for everything submitted."""
        for slot in self._slots:
            if slot.pending:
                slot.event.synchronize()
