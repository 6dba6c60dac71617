"""The optimiser step on the device: what every training loop of the reference runs after backward(),

    torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0);  optimizer.step();  optimizer.zero_grad()

with Adam, AdamW or SGD(momentum), optionally inside GradScaler.scale / unscale_ / step / update, as two launches over one
flat float32 buffer (include/optim/unetpp_optim.h, unet-_amd/csrc_optim/).  Nothing is read back and every result is bitwise
reproducible: chunking and reduction order follow from the element count alone.

* ``ParamArena`` moves a module's parameters into one flat buffer and attaches a flat gradient buffer as ``p.grad`` views.
* ``Adam``, ``AdamW``, ``SGD`` are ``torch.optim.Optimizer`` subclasses: ordinary ``param_groups`` (torch's schedulers drive
  them), torch's ``state_dict`` format, ``step()`` = two launches.  There is no CPU fallback: ``step()`` on a CPU arena raises.
* ``LossScaler`` is GradScaler's dynamic loss scale with scale and growth tracker on the device.
* ``grad_norm_np``, ``scalars_np``, ``step_np``, ``scaler_update_np``, ``pow_np`` are the NumPy form, float32 (float64 where
  the header says so) operation by operation: they define the device's arithmetic and the device tests compare bit for bit.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib_optim

# include/optim/unetpp_optim.h: unetpp_optim_layout reports the same numbers (tests/test_optim_bindings_host.py)
THREADS, GRANULE, MAX_PARTIALS, SLOT_WORDS, MAX_GROUPS, MAX_N = 256, 8192, 1024, 8, 8, 1 << 27
ST_STEP, ST_SCALE, ST_TRACKER, ST_NORM, ST_FOUND_INF = 0, 1, 2, 3, 4
KINDS = _lib_optim.KINDS
_F = np.float32
SET_TO_NONE = ("a parameter's .grad is no longer its view of the arena's flat gradient buffer; the usual cause is "
               "zero_grad(set_to_none=True) (torch's default): call the optimiser's or the arena's zero_grad(), or pass set_to_none=False")


# ------------------------------------------------------------------------------------------------------- the NumPy form
def chunk_for(n: int) -> int:
    """Elements per workgroup: a function of n alone."""
    per = GRANULE * MAX_PARTIALS
    return GRANULE * ((int(n) + per - 1) // per)


def parts_for(n: int) -> int:
    return (int(n) + chunk_for(n) - 1) // chunk_for(n)


def workspace_bytes(n: int) -> int:
    return parts_for(n) * 12


def grad_norm_np(g):
    """Launch A: (partial float64 [parts], flag uint32 [parts]) of the flat float32 gradients, in the kernel's order."""
    g = np.ascontiguousarray(g, dtype=np.float32).reshape(-1)
    n, chunk, parts = g.size, chunk_for(g.size), parts_for(g.size)
    iters = chunk // (4 * THREADS)
    x = np.zeros(parts * chunk, np.float64)
    x[:n] = g
    with np.errstate(all="ignore"):
        sq = (x * x).reshape(parts, iters, THREADS, 4)
        a = np.zeros((parts, THREADS, 4), np.float64)
        for it in range(iters):                                   # a thread's vectors in index order
            a = a + sq[:, it]
        v = ((a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])).reshape(parts, THREADS // 64, 64)
        off = 32
        while off:
            v[..., :off] = v[..., :off] + v[..., off:2 * off]
            off //= 2
        w = v[..., 0]
        partial = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    return partial, (~np.isfinite(partial)).astype(np.uint32)


def pow_np(b: float, e: int) -> float:
    """b ** e in float64 by square-and-multiply: the kernel's sequence of IEEE multiplications."""
    r, b, e = 1.0, float(b), int(e)
    while e:
        if e & 1:
            r = r * b
        e >>= 1
        if e:
            b = b * b
    return r


def group_doubles(group: dict, kind: str):
    """(lr, beta1, beta2, eps, weight_decay, momentum) of a param group as the doubles unetpp_optim_groups carries."""
    b1, b2 = group.get("betas", (0.0, 0.0))
    return (float(group["lr"]), float(b1), float(b2), float(group.get("eps", 0.0)), float(group.get("weight_decay", 0.0)),
            float(group.get("momentum", 0.0)) if kind == "sgd" else 0.0)


def scalars_np(partial, flag, step: int, groups, kind: str, max_norm=None, scale=None):
    """What every workgroup of launch B derives first.  scale: the loss scale (float32) with a scaler, None without."""
    S = 0.0
    for x in np.asarray(partial, np.float64).tolist():
        S = S + x
    with np.errstate(all="ignore"):
        inv_scale = _F(1) / _F(scale) if scale is not None else _F(1)
        total_norm = _F(np.sqrt(np.float64(S))) * inv_scale
        coef = _F(1)
        if max_norm is not None:
            coef = _F(max_norm) / (total_norm + _F(1e-6))
            if coef > _F(1):
                coef = _F(1)
        mult = inv_scale * coef
    t = int(step) + 1
    per_group = []
    for group in groups:
        lr, b1, b2, eps, wd, mu = group_doubles(group, kind)
        bc1, bc2 = 1.0 - pow_np(b1, t), 1.0 - pow_np(b2, t)
        with np.errstate(all="ignore"):
            ss = _F(np.float64(lr) / np.float64(bc1))
        per_group.append(dict(lr=_F(lr), wd=_F(wd), eps=_F(eps), mu=_F(mu), beta2=_F(b2), decay=_F(1.0 - lr * wd), omb1=_F(1.0 - b1),
                              omb2=_F(1.0 - b2), ss=ss, rbc2=_F(math.sqrt(bc2))))
    return dict(found_inf=bool(np.any(flag)), total_norm=total_norm, coef=coef, mult=mult, t=t, groups=per_group)


def scaler_update_np(scale, tracker: int, found_inf: bool, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
    """torch's _amp_update_scale_: (scale float32, tracker) after a step."""
    scale = _F(scale)
    if found_inf:
        return scale * _F(backoff_factor), 0
    if tracker + 1 == growth_interval:
        with np.errstate(all="ignore"):
            grown = scale * _F(growth_factor)
        return (grown if np.isfinite(grown) else scale), 0
    return scale, tracker + 1


def step_np(kind: str, p, g, m, v, groups, step: int, max_norm=None, scaler=None, zero_grads=False, norm=None):
    """Launch B on flat float32 arrays.  groups: dicts with "end" and the hyper-parameters of torch's param groups.  scaler:
    None or a dict(scale, tracker, growth_factor, backoff_factor, growth_interval).  norm: (partial, flag) of launch A, default
    grad_norm_np(g).  Returns dict(p, g, m, v, step, total_norm, found_inf, scale, tracker); the inputs are not changed."""
    p, g, m, v = (np.array(a, dtype=np.float32).reshape(-1) if a is not None else None for a in (p, g, m, v))
    partial, flag = norm if norm is not None else grad_norm_np(g)
    sc = scalars_np(partial, flag, step, groups, kind, max_norm, None if scaler is None else scaler["scale"])
    out = dict(total_norm=sc["total_norm"], found_inf=sc["found_inf"], scale=None, tracker=None)
    if scaler is not None:
        out["scale"], out["tracker"] = scaler_update_np(scaler["scale"], scaler["tracker"], sc["found_inf"], scaler["growth_factor"],
                                                        scaler["backoff_factor"], scaler["growth_interval"])
    skip = scaler is not None and sc["found_inf"]
    if not skip:
        start = 0
        with np.errstate(all="ignore"):
            for group, s in zip(groups, sc["groups"]):
                sl = slice(start, int(group["end"]))
                start = int(group["end"])
                gs = g[sl] * sc["mult"]
                if kind == "adamw":
                    if s["wd"] != 0:
                        p[sl] = p[sl] * s["decay"]
                elif s["wd"] != 0:
                    gs = gs + s["wd"] * p[sl]
                if kind == "sgd":
                    if s["mu"] != 0:
                        m[sl] = gs if sc["t"] == 1 else m[sl] * s["mu"] + gs
                        gs = m[sl]
                    p[sl] = p[sl] - s["lr"] * gs
                else:
                    m[sl] = m[sl] + (gs - m[sl]) * s["omb1"]
                    v[sl] = v[sl] * s["beta2"] + (gs * gs) * s["omb2"]
                    d = np.sqrt(v[sl]) / s["rbc2"] + s["eps"]
                    p[sl] = p[sl] - (s["ss"] * m[sl]) / d
    if zero_grads:
        g = np.zeros_like(g)
    out.update(p=p, g=g, m=m, v=v, step=int(step) if skip else sc["t"])
    return out


# ----------------------------------------------------------------------------------- the seeded scenes of the fixture
# tests/golden/optim_scenes.npz (scripts/make_golden_optim.py) holds torch's own CPU results on these; the tests regenerate the
# inputs from the seeds.  Four tensors in two param groups; every tensor starts at a multiple of 4 elements in the flat layout.
SCENE_SHAPES = ((8, 3, 3, 3), (8,), (24, 8, 3, 3), (13,))
SCENE_GROUP_OF = (0, 0, 1, 1)
SCENE_STEPS, SCENE_MAX_NORM = 20, 1.0
SCENES = {
    "adam": dict(kind="adam", seed=11, groups=[dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4),
                                               dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.0)]),
    "adamw": dict(kind="adamw", seed=12, groups=[dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2),
                                                 dict(lr=2e-3, betas=(0.9, 0.95), eps=1e-6, weight_decay=0.1)]),
    "sgd": dict(kind="sgd", seed=13, groups=[dict(lr=1e-2, momentum=0.9, weight_decay=1e-4), dict(lr=3e-2, momentum=0.9, weight_decay=0.0)]),
}
# the scaler scenes: the gradients arrive multiplied by the current scale; at OVERFLOW_STEPS one of them is +inf
SCALER = dict(init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2)
OVERFLOW_STEPS = (3, 11)
# the end-to-end scene: conv(3->8, 3x3, padding 1) - ReLU - conv(8->2, 1x1) on x [2,3,16,16], loss = E2E_LOSS_GAIN * mean(out^2)
E2E = dict(seed=21, steps=3, x_shape=(2, 3, 16, 16), loss_gain=200.0, groups=[dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)])


def scene_layout():
    """(offsets, ends, n) of SCENE_SHAPES in a ParamArena."""
    offsets, ends, n = [], [], 0
    for i, shape in enumerate(SCENE_SHAPES):
        if i and SCENE_GROUP_OF[i] != SCENE_GROUP_OF[i - 1]:
            ends.append(n)
        offsets.append(n)
        n += (int(np.prod(shape)) + 3) // 4 * 4
    return offsets, ends + [n], n


def scene_params(seed: int):
    """The initial parameters, one float32 array per tensor."""
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(s) * 0.2).astype(np.float32) for s in SCENE_SHAPES]


def scene_grads(seed: int, step: int):
    """The recorded gradients of step 0, 1, ...: the clip (SCENE_MAX_NORM) is active in two steps of three and idle in the third."""
    rng = np.random.default_rng(1000 * seed + step)
    amp = (0.1, 0.02, 0.005)[step % 3]
    return [(rng.standard_normal(s) * amp).astype(np.float32) for s in SCENE_SHAPES]


def flatten(tensors):
    """Per-tensor arrays -> the flat float32 layout of a ParamArena (zero padding)."""
    offsets, _, n = scene_layout()
    flat = np.zeros(n, np.float32)
    for t, o in zip(tensors, offsets):
        flat[o:o + t.size] = t.reshape(-1)
    return flat


def unflatten(flat):
    offsets, _, _ = scene_layout()
    return np.concatenate([flat[o:o + int(np.prod(s))] for o, s in zip(offsets, SCENE_SHAPES)])


def run_scene_np(name: str, scaler: bool = False):
    """SCENE_STEPS steps of step_np on a scene -> (final parameters without padding, [(scale, tracker) after each step])."""
    sc = SCENES[name]
    _, ends, n = scene_layout()
    groups = [dict(g, end=e) for g, e in zip(sc["groups"], ends)]
    p, m, v, step = flatten(scene_params(sc["seed"])), np.zeros(n, np.float32), np.zeros(n, np.float32), 0
    state = dict(SCALER, scale=_F(SCALER["init_scale"]), tracker=0) if scaler else None
    schedule = []
    for k in range(SCENE_STEPS):
        g = flatten(scene_grads(sc["seed"], k))
        if scaler:
            g = g * state["scale"]
            if k in OVERFLOW_STEPS:
                g[n // 2] = np.inf
        out = step_np(sc["kind"], p, g, m, v, groups, step, max_norm=SCENE_MAX_NORM, scaler=state)
        p, m, v, step = out["p"], out["m"], out["v"], out["step"]
        if scaler:
            state.update(scale=out["scale"], tracker=out["tracker"])
            schedule.append((float(out["scale"]), int(out["tracker"])))
    return unflatten(p), schedule


# ------------------------------------------------------------------------------------------------------------ the arena
def _torch():
    import torch
    return torch


def _as_groups(params_or_groups):
    items = list(params_or_groups)
    if not items:
        raise ValueError("ParamArena: no parameters")
    if not isinstance(items[0], dict):
        items = [{"params": items}]
    return [list(g["params"]) for g in items]


class ParamArena:
    """A module's parameters in one flat float32 buffer (``flat``), with a gradient buffer (``grad``) and two state buffers
    (``m``, ``v``) of the same layout.  ``p.data`` and ``p.grad`` become views; every parameter starts at a multiple of 4 elements
    (16 bytes) and the padding is zero and stays zero.  The parameters of a param group are one contiguous range; ``ends`` holds the
    groups' end offsets (the last is ``n``)."""

    def __init__(self, params_or_groups):
        torch = _torch()
        groups = _as_groups(params_or_groups)
        if len(groups) > MAX_GROUPS:
            raise ValueError(f"ParamArena: {len(groups)} param groups, at most {MAX_GROUPS}")
        self.params, self.offsets, self.ends = [], [], []
        n = 0
        for params in groups:
            for p in params:
                if p.dtype != torch.float32:
                    raise TypeError(f"ParamArena: float32 parameters only, got {p.dtype}")
                if any(p is q for q in self.params):
                    raise ValueError("ParamArena: a parameter appears twice")
                if self.params and p.device != self.params[0].device:
                    raise ValueError("ParamArena: parameters on different devices")
                self.params.append(p)
                self.offsets.append(n)
                n += (p.numel() + 3) // 4 * 4
            if n == (self.ends[-1] if self.ends else 0):
                raise ValueError("ParamArena: an empty param group")
            self.ends.append(n)
        if not 1 <= n <= MAX_N:
            raise ValueError(f"ParamArena: {n} elements, the kernels take 1 .. {MAX_N}")
        self.n, self.device = n, self.params[0].device
        self.flat, self.grad, self.m, self.v = (torch.zeros(n, dtype=torch.float32, device=self.device) for _ in range(4))
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                view = self.flat[o:o + p.numel()].view(p.shape)
                view.copy_(p.data)
                gview = self.grad[o:o + p.numel()].view(p.shape)
                if p.grad is not None:
                    gview.copy_(p.grad)
                p.data = view
                p.grad = gview

    def views(self, flat, i):
        """Parameter i's view of one of the flat buffers."""
        p, o = self.params[i], self.offsets[i]
        return flat[o:o + p.numel()].view(p.shape)

    def zero_grad(self):
        """One memset; the ``p.grad`` views stay attached."""
        self.grad.zero_()

    def check(self):
        """Host-side, by data_ptr: every ``p.data`` and ``p.grad`` is still its view.  Reads nothing from the device."""
        base, gbase = self.flat.data_ptr(), self.grad.data_ptr()
        for p, o in zip(self.params, self.offsets):
            if p.grad is None or p.grad.data_ptr() != gbase + 4 * o or not p.grad.is_contiguous():
                raise RuntimeError("ParamArena: " + SET_TO_NONE)
            if p.data_ptr() != base + 4 * o:
                raise RuntimeError("ParamArena: a parameter's .data was replaced and is no longer its view of the arena's flat buffer")


# ----------------------------------------------------------------------------------------------------------- the scaler
def _new_state(torch, device):
    return torch.zeros(2 * SLOT_WORDS, dtype=torch.int32, device=device)


class LossScaler:
    """GradScaler's dynamic loss scale with the scale and the growth tracker on the device.  ``scale(loss)`` multiplies by a
    device scalar; ``optimizer.step(scaler=...)`` takes the place of ``unscale_`` + clip + ``step`` + ``update`` (one optimiser per
    scaler).  Only ``get_scale()`` and ``state_dict()`` read back."""

    def __init__(self, device="cuda", init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        torch = _torch()
        if not (growth_factor > 1.0 and 0.0 < backoff_factor < 1.0 and int(growth_interval) >= 1):
            raise ValueError("LossScaler: growth_factor > 1, 0 < backoff_factor < 1, growth_interval >= 1")
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self._state = _new_state(torch, torch.device(device))
        self.device = self._state.device                           # "cuda" resolved to the current device's index
        self._parity = 0
        self._set(init_scale, 0)

    def _set(self, scale, tracker):
        torch = _torch()
        slot = torch.zeros(SLOT_WORDS, dtype=torch.int32)
        slot[ST_SCALE] = int(np.float32(scale).view(np.int32))
        slot[ST_TRACKER] = int(tracker)
        self._state[self._parity * SLOT_WORDS:(self._parity + 1) * SLOT_WORDS].copy_(slot)

    def _slot(self):
        return self._state[self._parity * SLOT_WORDS:(self._parity + 1) * SLOT_WORDS]

    def scale_tensor(self):
        """The current scale as a 0-dim float32 view on the device (valid until the next step)."""
        torch = _torch()
        return self._slot()[ST_SCALE:ST_SCALE + 1].view(torch.float32)[0]

    def scale(self, loss):
        return loss * self.scale_tensor()

    def get_scale(self) -> float:
        return float(self.scale_tensor().item())

    def state_dict(self) -> dict:
        """torch.amp.GradScaler's format."""
        slot = self._slot().cpu()
        return {"scale": float(slot[ST_SCALE:ST_SCALE + 1].view(_torch().float32)[0]), "growth_factor": self.growth_factor,
                "backoff_factor": self.backoff_factor, "growth_interval": self.growth_interval, "_growth_tracker": int(slot[ST_TRACKER])}

    def load_state_dict(self, sd: dict):
        self.growth_factor, self.backoff_factor, self.growth_interval = float(sd["growth_factor"]), float(sd["backoff_factor"]), int(sd["growth_interval"])
        self._set(sd["scale"], sd["_growth_tracker"])


# ------------------------------------------------------------------------------------------------------- the optimisers
def _base():
    torch = _torch()

    class ArenaOptimizer(torch.optim.Optimizer):
        """Shared part of Adam / AdamW / SGD below."""
        kind, torch_class = None, None

        def __init__(self, params, max_norm=None, zero_grads=False, check=True, **hyper):
            arena = params if isinstance(params, ParamArena) else None
            if arena is not None:
                starts = [0] + arena.ends[:-1]
                params = [{"params": [p for p, o in zip(arena.params, arena.offsets) if a <= o < b]} for a, b in zip(starts, arena.ends)]
            template = self.torch_class([torch.nn.Parameter(torch.zeros(1))], **hyper)     # torch validates the hyper-parameters
            super().__init__(params, dict(template.defaults))
            for g in self.param_groups:
                if g.get("amsgrad") or g.get("nesterov") or g.get("maximize") or g.get("dampening"):
                    raise ValueError("amsgrad, nesterov, maximize and dampening are not supported")
            self.arena = arena if arena is not None else ParamArena(self.param_groups)
            if max_norm is not None and not float(max_norm) > 0:
                raise ValueError("max_norm must be positive or None")
            self.max_norm, self.zero_grads, self.check_views = (None if max_norm is None else float(max_norm)), bool(zero_grads), bool(check)
            self._dev_state = _new_state(torch, self.arena.device)
            self._parity = 0
            self._workspace = torch.zeros((workspace_bytes(self.arena.n) + 7) // 8, dtype=torch.float64, device=self.arena.device)
            self._groups, self._args = _lib_optim.Groups(), _lib_optim.StepArgs()

        # -- the step
        def _fill_groups(self):
            G = self._groups
            G.n_groups, G.kind = len(self.param_groups), KINDS[self.kind]
            for k, (group, end) in enumerate(zip(self.param_groups, self.arena.ends)):
                G.end[k] = end
                G.lr[k], G.beta1[k], G.beta2[k], G.eps[k], G.weight_decay[k], G.momentum[k] = group_doubles(group, self.kind)
            return G

        @torch.no_grad()
        def step(self, closure=None, scaler=None):
            """clip (with max_norm) + update (+ zero the gradients with zero_grads) in two launches on the current stream.  With
            ``scaler`` also unscale, skip on a non-finite gradient, and update the scale; nothing is read back."""
            loss = None
            if closure is not None:
                with torch.enable_grad():
                    loss = closure()
            a = self.arena
            if a.device.type != "cuda":
                raise RuntimeError("unet_amd.optim: step() runs on the device only; there is no CPU fallback")
            if self.check_views:
                a.check()
            lib = _lib_optim.load()
            A = self._args
            A.use_clip, A.max_norm = int(self.max_norm is not None), float(self.max_norm or 0.0)
            A.zero_grads, A.parity = int(self.zero_grads), self._parity
            scaler_ptr = None
            if scaler is not None:
                if scaler.device != a.device:
                    raise ValueError(f"the scaler is on {scaler.device}, the parameters on {a.device}")
                A.growth_factor, A.backoff_factor, A.growth_interval = scaler.growth_factor, scaler.backoff_factor, scaler.growth_interval
                A.scaler_parity = scaler._parity
                scaler_ptr = scaler._state.data_ptr()
            else:
                A.growth_factor, A.backoff_factor, A.growth_interval, A.scaler_parity = 1.0, 1.0, 1, 0
            with torch.cuda.device(a.device):
                stream = torch.cuda.current_stream().cuda_stream
                rc = lib.unetpp_optim_grad_norm_f32(a.grad.data_ptr(), a.n, self._workspace.data_ptr(), stream)
                if rc:
                    raise RuntimeError(f"unetpp_optim_grad_norm_f32: {rc}")
                sgd = self.kind == "sgd"
                rc = lib.unetpp_optim_step_f32(a.flat.data_ptr(), a.grad.data_ptr(), a.m.data_ptr(), None if sgd else a.v.data_ptr(), a.n,
                                               ctypes.byref(self._fill_groups()), ctypes.byref(A), self._workspace.data_ptr(),
                                               self._dev_state.data_ptr(), scaler_ptr, stream)
                if rc:
                    raise RuntimeError(f"unetpp_optim_step_f32: {rc}")
            self._parity ^= 1
            if scaler is not None:
                scaler._parity ^= 1
            return loss

        def zero_grad(self, set_to_none=False):
            if set_to_none:
                raise RuntimeError("unet_amd.optim: zero_grad(set_to_none=True) would detach the gradients from the arena; " + SET_TO_NONE)
            self.arena.zero_grad()

        def add_param_group(self, param_group):
            if hasattr(self, "arena"):
                raise RuntimeError("unet_amd.optim: param groups are fixed once the arena is built")
            super().add_param_group(param_group)

        # -- the state, in torch's format
        def _slot(self):
            return self._dev_state[self._parity * SLOT_WORDS:(self._parity + 1) * SLOT_WORDS]

        def step_count(self) -> int:
            """Reads back."""
            return int(self._slot()[ST_STEP].item())

        def total_norm(self) -> float:
            """The gradient norm of the last step (what clip_grad_norm_ returns).  Reads back."""
            return float(self._slot()[ST_NORM:ST_NORM + 1].view(torch.float32)[0].item())

        def state_dict(self):
            """torch's format: per parameter exp_avg, exp_avg_sq and step, or momentum_buffer.  The one place that reads back."""
            a, step = self.arena, self.step_count()
            self.state.clear()
            if step > 0:
                for i, p in enumerate(a.params):
                    if self.kind == "sgd":
                        if any(g.get("momentum", 0) for g in self.param_groups):
                            self.state[p] = {"momentum_buffer": a.views(a.m, i).clone()}
                    else:
                        self.state[p] = {"step": torch.tensor(float(step)), "exp_avg": a.views(a.m, i).clone(), "exp_avg_sq": a.views(a.v, i).clone()}
            try:
                return super().state_dict()
            finally:
                self.state.clear()

        def load_state_dict(self, state_dict):
            a = self.arena
            super().load_state_dict(state_dict)
            step = 0
            a.m.zero_()
            a.v.zero_()
            for i, p in enumerate(a.params):
                st = self.state.get(p, {})
                if self.kind == "sgd":
                    if st.get("momentum_buffer") is not None:
                        a.views(a.m, i).copy_(st["momentum_buffer"])
                        step = max(step, 1)
                elif st:
                    a.views(a.m, i).copy_(st["exp_avg"])
                    a.views(a.v, i).copy_(st["exp_avg_sq"])
                    step = max(step, int(float(st["step"])))
            self.state.clear()
            slot = torch.zeros(SLOT_WORDS, dtype=torch.int32)
            slot[ST_STEP] = step
            self._slot().copy_(slot)

    return ArenaOptimizer


_classes = {}


def _torch_classes():
    """Adam, AdamW and SGD, defined on first use: they derive from torch.optim.Optimizer, and importing this module needs no
    torch (the NumPy form runs without it)."""
    if not _classes:
        torch, base = _torch(), _base()
        doc = ("torch.optim.%s on a ParamArena: the reference's keywords plus max_norm=None (clip_grad_norm_'s), zero_grads=False "
               "(zero the gradients in the step) and check=True (arena.check() before every step).")
        for name, kind in (("Adam", "adam"), ("AdamW", "adamw"), ("SGD", "sgd")):
            _classes[name] = type(name, (base,), {"kind": kind, "torch_class": getattr(torch.optim, name), "__doc__": doc % name,
                                                  "__module__": __name__})
    return _classes


def __getattr__(name):
    if name in ("Adam", "AdamW", "SGD"):
        return _torch_classes()[name]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
