"""Guard-band placement for the device tests: every tensor a kernel may touch lies in an arena of its own,
``[guard | payload | guard]``, filled with seeded random bytes, and the guards are compared with their pattern afterwards.

* ``Guard.place(array, offset)`` puts an input at a chosen address modulo 16 (odd for uint8, 4 for float32 / int32, ...).
* ``Guard.allocations()`` patches ``torch.empty`` / ``torch.zeros`` / ``torch.empty_like`` so that every output and
  workspace the wrappers allocate is carved from an arena, at the alignment include/unetpp.h promises and no better, and
  wraps ``PostProcessing._call`` so that a tensor reaching the library from anywhere else fails the test.
* ``Guard.check()`` names the arena, the side and the first and last changed offset of every damaged guard.
* ``two_fillings(fn)`` runs ``fn`` with filling A and with its complement and demands bitwise equal results: a kernel
  that READS a neighbour and lets the value reach its result is caught, and so is output that was never written (the
  payload of an output arena is random too).

The module is a plain helper (no fixtures, no pytest hooks) and works on CPU tensors as well: tests/test_guarded_host.py
proves there that each of its checks can fail."""
import contextlib

import numpy as np

MIN_GUARD = 4096
NETWORK, WORKSPACE = "network", "workspace"


class GuardError(AssertionError):
    pass


class Arena:
    """One uint8 allocation [guard | payload | guard]; `lo` .. `hi` are the payload's byte offsets in it."""

    def __init__(self, torch, name, nbytes, row_bytes, offset, device, rng, complement, raw_alloc):
        guard = max(MIN_GUARD, 2 * int(row_bytes))
        self.name, self.nbytes = name, int(nbytes)
        total = guard + 16 + self.nbytes + guard
        self.buf = raw_alloc(total, dtype=torch.uint8, device=device)
        self.lo = guard + (int(offset) - (self.buf.data_ptr() + guard)) % 16          # payload address = offset (mod 16)
        self.hi = self.lo + self.nbytes
        fill = rng.integers(0, 256, total, dtype=np.uint8)
        if complement:
            fill = ~fill
        self.pattern = fill
        self.buf.copy_(torch.from_numpy(fill))
        self.base = self.buf.data_ptr()

    def payload(self):
        return self.buf[self.lo:self.hi]

    def holds(self, ptr, nbytes):
        return self.base + self.lo <= ptr and ptr + nbytes <= self.base + self.hi

    def damage(self):
        """[(side, first, last)] of the changed guard bytes, offsets relative to the payload's first byte."""
        now = self.buf.cpu().numpy()
        bad = []
        for side, a, b in (("front", 0, self.lo), ("back", self.hi, now.size)):
            diff = np.flatnonzero(now[a:b] != self.pattern[a:b])
            if diff.size:
                bad.append((side, int(diff[0]) + a - self.lo, int(diff[-1]) + a - self.lo))
        return bad


# what a tensor of each element size gets by default: the least include/unetpp.h promises the kernels
_CONTRACT = {1: 0, 2: 2, 4: 4, 8: 8}


class Guard:
    def __init__(self, torch, device="cuda", seed=0, complement=False, u8_out_offset=0, align=None):
        """u8_out_offset: the address modulo 16 of uint8 outputs (1 = one byte off).  align(shape, dtype, contexts) may
        return an offset for one allocation (None: the default), for the few buffers whose contract is stricter."""
        self.torch, self.device = torch, torch.device(device)
        self.rng = np.random.default_rng(seed)
        self.complement, self.u8_out_offset, self.align = bool(complement), int(u8_out_offset), align
        self.arenas, self.calls, self.symbols, self.contexts = [], [], [], []
        self.exempt = set()                       # {(entry, argument position)}: stated exemptions of the completeness hook
        self._raw = {n: getattr(torch, n) for n in ("empty", "zeros", "empty_like")}

    # ---- arenas
    def _arena(self, name, shape, dtype, offset):
        torch = self.torch
        item = torch.empty((), dtype=dtype).element_size()
        n = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
        row = (shape[-1] if len(shape) else 1) * item
        if len(shape) == 4 and shape[-1] <= 4:
            row *= shape[-2]                     # [B,H,W,3]: a row is W pixels
        a = Arena(torch, name, n * item, row, offset, self.device, self.rng, self.complement, self._raw["empty"])
        self.arenas.append(a)
        return a, a.payload().view(dtype).view(tuple(shape))

    def place(self, array, offset=0, name=None):
        """A contiguous device view holding `array` whose first byte lies at `offset` modulo 16."""
        torch = self.torch
        array = np.ascontiguousarray(array)
        if offset % array.dtype.itemsize:
            raise ValueError(f"offset {offset} is not a multiple of the element size {array.dtype.itemsize}")
        t = torch.from_numpy(array)
        _, view = self._arena(name or f"input{len(self.arenas)}", tuple(array.shape), t.dtype, offset)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 16 == offset % 16
        return view

    def _offset_for(self, shape, dtype):
        torch = self.torch
        if self.align is not None:
            got = self.align(tuple(shape), dtype, tuple(self.contexts))
            if got is not None:
                return int(got)
        if WORKSPACE in self.contexts:
            return 0
        item = torch.empty((), dtype=dtype).element_size()
        if NETWORK in self.contexts:
            return 0 if item == 4 else 4          # logits and probabilities 16, the masks 4 (unetpp_forward_ds)
        if item == 1:
            return self.u8_out_offset
        return _CONTRACT.get(item, 0)

    def alloc(self, shape, dtype, zero=False, name=None):
        offset = self._offset_for(shape, dtype)
        a, view = self._arena(name or f"alloc{len(self.arenas)}:{tuple(shape)}:{dtype}", tuple(shape), dtype, offset)
        assert view.is_contiguous() and (view.numel() == 0 or view.data_ptr() % 16 == offset % 16)
        if zero:
            view.zero_()
        return view

    def find(self, t):
        n = t.numel() * t.element_size()
        for a in self.arenas:
            if a.holds(t.data_ptr(), n):
                return a
        return None

    def require_inside(self, t, what):
        if t.numel() and self.find(t) is None:
            raise GuardError(f"{what}: a tensor {tuple(t.shape)} {t.dtype} that is not wholly inside a live arena's payload")

    def check(self):
        bad = [f"arena {a.name!r} ({a.nbytes} bytes): {side} guard changed, payload-relative offsets {first} .. {last}"
               for a in self.arenas for side, first, last in a.damage()]
        if bad:
            raise GuardError("guard bytes were written:\n  " + "\n  ".join(bad))

    # ---- the allocation patch and the completeness hook
    def _mine(self, device):
        return device is not None and self.torch.device(device).type == self.device.type

    @contextlib.contextmanager
    def context(self, tag):
        self.contexts.append(tag)
        try:
            yield
        finally:
            self.contexts.pop()

    @contextlib.contextmanager
    def allocations(self, call_owner=None, models=(), lib_module=None):
        """Patch the allocation forms the wrappers use; wrap call_owner._call (default PostProcessing) and _workspace, the
        network's direct library calls of every model in `models`' classes, and, with lib_module (unet_amd._lib), record
        every library symbol called.  The workspace caches of `models` are emptied on entry and exit: a cached buffer
        would outlive its arena."""
        torch, guard = self.torch, self
        raw = self._raw

        def shape_of(args, kwargs):
            if "size" in kwargs:
                return tuple(kwargs["size"])
            if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
                return tuple(args[0])
            return tuple(int(a) for a in args)

        def make(zero):
            def patched(*args, **kwargs):
                if not guard._mine(kwargs.get("device")) or kwargs.get("out") is not None:
                    return raw["zeros" if zero else "empty"](*args, **kwargs)
                dtype = kwargs.get("dtype") or torch.get_default_dtype()
                return guard.alloc(shape_of(args, kwargs), dtype, zero)
            return patched

        def empty_like(t, **kwargs):
            device = kwargs.get("device", t.device)
            if not guard._mine(device):
                return raw["empty_like"](t, **kwargs)
            return guard.alloc(tuple(t.shape), kwargs.get("dtype") or t.dtype)

        if call_owner is None:
            from unet_amd.postproc import PostProcessing as call_owner
        orig_call = call_owner._call
        orig_ws = getattr(call_owner, "_workspace", None)

        def hooked_call(model, name, *args, **kwargs):
            for pos, a in enumerate(args):
                if isinstance(a, torch.Tensor) and (name, pos) not in guard.exempt:
                    guard.require_inside(a, f"{name}, argument {pos}")
            guard.calls.append(name)
            return orig_call(model, name, *args, **kwargs)

        def hooked_ws(model, *args, **kwargs):
            with guard.context(WORKSPACE):
                return orig_ws(model, *args, **kwargs)

        restore = [(call_owner, "_call", orig_call)]
        call_owner._call = hooked_call
        if orig_ws is not None:
            restore.append((call_owner, "_workspace", orig_ws))
            call_owner._workspace = hooked_ws

        def flat(r):
            if isinstance(r, torch.Tensor):
                yield r
            elif isinstance(r, (tuple, list)):
                for v in r:
                    yield from flat(v)

        def network(cls, method):
            orig = getattr(cls, method)

            def run(model, *args, **kwargs):
                with guard.context(NETWORK):
                    out = orig(model, *args, **kwargs)
                for i, t in enumerate(flat(out)):
                    guard.require_inside(t, f"{method}, result {i}")
                return out
            restore.append((cls, method, orig))
            setattr(cls, method, run)

        for cls in {c for m in models for c in type(m).__mro__ if "_run" in vars(c) or "forward_deep_supervision" in vars(c)}:
            for method in ("_run", "forward_deep_supervision"):
                if method in vars(cls):
                    network(cls, method)

        class Recorder:
            def __init__(self, lib):
                self._lib = lib

            def __getattr__(self, name):
                fn = getattr(self._lib, name)
                if not name.startswith("unetpp_"):
                    return fn

                def call(*args):
                    guard.symbols.append(name)
                    return fn(*args)
                return call

        real_lib = None
        if lib_module is not None:
            real_lib = lib_module.load()
            lib_module._lib = Recorder(real_lib)
        for m in models:
            m._cc_workspaces.clear()
        torch.empty, torch.zeros, torch.empty_like = make(False), make(True), empty_like
        try:
            yield self
        finally:
            torch.empty, torch.zeros, torch.empty_like = raw["empty"], raw["zeros"], raw["empty_like"]
            for owner, attr, orig in restore:
                setattr(owner, attr, orig)
            if lib_module is not None:
                lib_module._lib = real_lib
            for m in models:
                m._cc_workspaces.clear()


def as_bytes(torch, r):
    """The results of a call as a flat list of (path, numpy array of raw bytes + dtype + shape): what 'bitwise equal' compares."""
    out = []

    def walk(path, v):
        if isinstance(v, torch.Tensor):
            a = v.detach().cpu().contiguous()
            if a.dtype == torch.bool:
                a = a.to(torch.uint8)
            a = a.numpy()
            out.append((path, str(a.dtype), a.shape, np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()))
        elif isinstance(v, dict):
            for k in sorted(v):
                walk(f"{path}[{k!r}]", v[k])
        elif isinstance(v, (tuple, list)):
            for i, x in enumerate(v):
                walk(f"{path}[{i}]", x)
        elif isinstance(v, np.ndarray):
            out.append((path, str(v.dtype), v.shape, np.ascontiguousarray(v).view(np.uint8).reshape(-1).copy()))
        else:
            out.append((path, type(v).__name__, (), np.frombuffer(repr(v).encode(), np.uint8).copy()))
    walk("result", r)
    return out


def assert_same_bytes(a, b, what):
    assert len(a) == len(b), f"{what}: {len(a)} results against {len(b)}"
    for (pa, da, sa, xa), (pb, db, sb, xb) in zip(a, b):
        assert (pa, da, sa) == (pb, db, sb), f"{what}: {pa} {da} {sa} against {pb} {db} {sb}"
        if not np.array_equal(xa, xb):
            diff = np.flatnonzero(xa != xb)
            raise GuardError(f"{what}: {pa} ({da} {sa}) differs in {diff.size} bytes, first at byte {int(diff[0])}")


def two_fillings(torch, run, device="cuda", seed=0, **guard_kw):
    """run(guard) -> results, once with filling A and once with its bitwise complement; the guards are checked after
    each run and the two results must be bitwise equal.  Returns the first run's results (as as_bytes gives them)."""
    got = []
    for complement in (False, True):
        g = Guard(torch, device, seed, complement, **guard_kw)
        r = run(g)
        if g.device.type == "cuda":
            torch.cuda.synchronize()
        got.append(as_bytes(torch, r))
        g.check()
    try:
        assert_same_bytes(got[0], got[1], "the two guard fillings")
    except AssertionError as e:
        raise GuardError(f"{e}: the result depends on bytes outside the tensors, or a part of an output was never written") from None
    return got[0]
