"""The optimiser step on the device (include/optim/unetpp_optim.h) against its NumPy form (unet_amd/optim.py), bit for bit.

  step        launch B equals step_np in p, m, v, g (float32 compared as int32) and in the state words, given the table launch A
              produced: every kind; clip off, far below and far above the norm; scaler on and off; zero_grads on and off; step
              counts 1, 2 and 1000; n in SIZES (the vector tail, chunk - 1 / chunk / chunk + 1, several chunks); group
              boundaries inside a 4-element vector and across a chunk boundary; gradients with subnormals, squares that underflow, +-0
  norm        launch A's table equals grad_norm_np's, the float32 norm lies within 1 ulp of the exactly rounded one, two runs are
              bitwise identical, and so is a run on the gradients at another base address (16 bytes on; 4 bytes on: the narrow path)
  non-finite  with the scaler p, m, v and the step count stay, the scale halves, and doubles after growth_interval = 2 clean steps,
              five launches in a row (both state slots); without it the result equals torch's CPU result, NaNs by position
  end to end  the public classes: ParamArena + AdamW(max_norm) + LossScaler on the fixture's scenes and on a two-conv module
Run on the GPU box:  python -m pytest tests/test_gpu_optim.py -m gpu"""
import ctypes
import math

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import _lib_optim, optim

C = optim.GRANULE
SIZES = [1, 3, 4, 5, 1023, C - 1, C, C + 1, 3 * C + 7]
KINDS = ["adam", "adamw", "sgd"]
HYPER = {"adam": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2), "adamw": dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1),
         "sgd": dict(lr=1e-2, momentum=0.9, weight_decay=1e-3)}
SCALER = dict(growth_factor=2.0, backoff_factor=0.5, growth_interval=2)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "the gpu tests need a HIP device"
    return torch


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def two_groups(kind, ends):
    """Param groups with different hyper-parameters ending at `ends`."""
    out = []
    for k, end in enumerate(ends):
        g = dict(HYPER[kind], end=int(end))
        g["lr"] = g["lr"] * (1 + k)
        if k % 2:
            g["weight_decay"] = 0.0
        out.append(g)
    return out


def tensors(n, seed, step):
    """(p, g, m, v): wide magnitudes, and among the gradients subnormals, values whose float32 square underflows, and +-0."""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(n) * np.exp(rng.uniform(-6, 2, n))).astype(np.float32)
    g = (rng.standard_normal(n) * np.exp(rng.uniform(-12, 3, n))).astype(np.float32)
    special = np.float32([1e-40, -3e-42, 1e-30, -2e-25, 0.0, -0.0, 1e-20])
    where = rng.random(n) < 0.3
    g[where] = rng.choice(special, int(where.sum()))
    p[rng.random(n) < 0.05] = np.float32(2e-41)
    g[0] = np.float32(3.5 + seed % 3)                                      # the norm is at least this, whatever n
    if step == 0:
        return p, g, np.zeros(n, np.float32), np.zeros(n, np.float32)
    m = (rng.standard_normal(n) * 0.1).astype(np.float32)
    v = (rng.standard_normal(n) * 0.1).astype(np.float32) ** 2
    return p, g, m, v


class DeviceRun:
    """The two launches on caller-placed tensors, with the host-side parities of optim.py."""

    def __init__(self, torch, kind, p, m, v, groups, step=0, scaler=None, place=None):
        self.torch, self.kind, self.groups, self.n = torch, kind, groups, p.size
        self.place = place or (lambda a, what: torch.from_numpy(np.ascontiguousarray(a)).cuda())
        self.p, self.m = self.place(p, "p"), self.place(m, "m")
        self.v = None if kind == "sgd" else self.place(v, "v")
        self.workspace = self.place(np.zeros((optim.workspace_bytes(self.n) + 7) // 8, np.float64), "workspace")
        state = np.zeros(2 * optim.SLOT_WORDS, np.int32)
        state[optim.ST_STEP] = step
        self.state, self.parity = self.place(state, "state"), 0
        self.scaler_state, self.scaler_parity, self.scaler = None, 0, scaler
        if scaler is not None:
            s = np.zeros(2 * optim.SLOT_WORDS, np.int32)
            s[optim.ST_SCALE], s[optim.ST_TRACKER] = np.float32(scaler["scale"]).view(np.int32), scaler["tracker"]
            self.scaler_state = self.place(s, "scaler_state")
        self.G = _lib_optim.Groups()
        self.G.n_groups, self.G.kind = len(groups), optim.KINDS[kind]
        for k, grp in enumerate(groups):
            self.G.end[k] = grp["end"]
            self.G.lr[k], self.G.beta1[k], self.G.beta2[k], self.G.eps[k], self.G.weight_decay[k], self.G.momentum[k] = optim.group_doubles(grp, kind)

    def norm(self, g_dev):
        rc = _lib_optim.load().unetpp_optim_grad_norm_f32(g_dev.data_ptr(), self.n, self.workspace.data_ptr(), None)
        assert rc == 0, rc

    def table(self):
        parts = optim.parts_for(self.n)
        raw = self.workspace.cpu().numpy().view(np.uint8)[:12 * parts]
        return raw[:8 * parts].view(np.float64).copy(), raw[8 * parts:].view(np.uint32).copy()

    def run(self, g, max_norm=None, zero_grads=False):
        """Both launches on gradients g; -> what the device holds afterwards (and this run's table)."""
        torch = self.torch
        g_dev = g if isinstance(g, torch.Tensor) else self.place(g, "g")
        self.norm(g_dev)
        A = _lib_optim.StepArgs()
        A.use_clip, A.max_norm, A.zero_grads = int(max_norm is not None), float(max_norm or 0.0), int(zero_grads)
        A.parity, A.scaler_parity = self.parity, self.scaler_parity
        if self.scaler is not None:
            A.growth_factor, A.backoff_factor, A.growth_interval = (self.scaler[k] for k in ("growth_factor", "backoff_factor", "growth_interval"))
        rc = _lib_optim.load().unetpp_optim_step_f32(
            self.p.data_ptr(), g_dev.data_ptr(), self.m.data_ptr(), None if self.v is None else self.v.data_ptr(), self.n, ctypes.byref(self.G),
            ctypes.byref(A), self.workspace.data_ptr(), self.state.data_ptr(), None if self.scaler_state is None else self.scaler_state.data_ptr(), None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        self.parity ^= 1
        slot = self.state.cpu().numpy()[self.parity * optim.SLOT_WORDS:][:optim.SLOT_WORDS]
        out = dict(p=self.p.cpu().numpy(), g=g_dev.cpu().numpy(), m=self.m.cpu().numpy(), v=None if self.v is None else self.v.cpu().numpy(),
                   step=int(slot[optim.ST_STEP]), total_norm=slot[optim.ST_NORM:optim.ST_NORM + 1].view(np.float32)[0],
                   found_inf=bool(slot[optim.ST_FOUND_INF]), table=self.table(), scale=None, tracker=None)
        if self.scaler_state is not None:
            self.scaler_parity ^= 1
            s = self.scaler_state.cpu().numpy()[self.scaler_parity * optim.SLOT_WORDS:][:optim.SLOT_WORDS]
            out["scale"], out["tracker"] = s[optim.ST_SCALE:optim.ST_SCALE + 1].view(np.float32)[0], int(s[optim.ST_TRACKER])
        return out


def assert_equals_form(got, want, what):
    """A DeviceRun.run result against step_np's, float32 as int32."""
    for k in ("p", "m", "v", "g"):
        if got[k] is not None:
            diff = np.flatnonzero(bits(got[k]) != bits(want[k]))
            assert diff.size == 0, f"{what}: {k} differs in {diff.size} elements, first at {int(diff[0])}: {got[k][diff[0]]!r} != {want[k][diff[0]]!r}"
    assert got["step"] == want["step"] and got["found_inf"] == want["found_inf"], what
    assert bits(got["total_norm"]) == bits(want["total_norm"]) or (np.isnan(got["total_norm"]) and np.isnan(want["total_norm"])), what
    if want["scale"] is not None:
        assert bits(got["scale"]) == bits(want["scale"]) and got["tracker"] == want["tracker"], what


def check_case(torch, kind, n, groups, seed, step, max_norm, use_scaler, zero_grads, place=None):
    p, g, m, v = tensors(n, seed, step)
    scaler = dict(SCALER, scale=np.float32(1024.0), tracker=seed % 2) if use_scaler else None
    if use_scaler:
        g = g * np.float32(1024.0)
    run = DeviceRun(torch, kind, p, m, v, groups, step, scaler, place)
    got = run.run(g, max_norm, zero_grads)
    want = optim.step_np(kind, p, g, m, v, groups, step, max_norm=max_norm, scaler=scaler, zero_grads=zero_grads, norm=got["table"])
    what = f"{kind} n={n} step={step} max_norm={max_norm} scaler={use_scaler} zero_grads={zero_grads}"
    assert_equals_form(got, want, what)
    if not zero_grads:
        assert bits(got["g"]).tobytes() == bits(g).tobytes(), what + ": the gradients were written"
    return got, want


# the norm of tensors() is at least 3.5 (its first element) and far below 1e12, so 1e-3 always clips and 1e12 never does
CLIPS = [None, 1e-3, 1e12]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_step_equals_the_numpy_form_bit_for_bit(torch_cuda, kind, n):
    groups = two_groups(kind, [n // 2, n] if n >= 2 else [n])              # n = 3, 5, 1023: the boundary inside a vector
    i, active = 0, []
    for max_norm in CLIPS:
        for use_scaler in (False, True):
            for zero_grads in (False, True):
                step = (0, 1, 999)[i % 3]
                got, want = check_case(torch_cuda, kind, n, groups, 100 * n + i, step, max_norm, use_scaler, zero_grads)
                active.append(optim.scalars_np(*got["table"], step, groups, kind, max_norm, np.float32(1024) if use_scaler else None)["coef"] < 1)
                i += 1
    assert active == [False] * 4 + [True] * 4 + [False] * 4                # the clip was idle, active, idle as intended


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_group_boundaries_inside_a_vector_and_across_a_chunk(torch_cuda, kind):
    n = C + 100
    for ends in ([5, 4098, C + 3, n], [1, 2, 3, 6, 7, C - 1, C, n], [C - 2, C + 2, n]):
        for step, max_norm, use_scaler in ((0, 1e-3, False), (999, None, True)):
            check_case(torch_cuda, kind, n, two_groups(kind, ends), len(ends), step, max_norm, use_scaler, True)


def ulps(a, b):
    return abs(int(bits(a).reshape(-1)[0]) - int(bits(b).reshape(-1)[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_norm_is_exact_to_one_ulp_reproducible_and_independent_of_the_address(torch_cuda, n):
    torch = torch_cuda
    _, g, _, _ = tensors(n, 7 * n, 0)
    run = DeviceRun(torch, "adam", g, g, g, two_groups("adam", [n]))
    buf = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    tables = []
    for start in (0, 0, 4, 1, 3):                                          # twice the same; 16 bytes on; 4 and 12 bytes on (4-byte accesses)
        view = buf[start:start + n]
        view.copy_(torch.from_numpy(g))
        assert view.data_ptr() % 16 == (4 * start) % 16
        run.workspace.zero_()
        run.norm(view)
        torch.cuda.synchronize()
        tables.append(run.table())
    want = optim.grad_norm_np(g)
    for partial, flag in tables:
        assert partial.view(np.int64).tobytes() == want[0].view(np.int64).tobytes() and flag.tobytes() == want[1].tobytes()
    exact = math.sqrt(math.fsum(float(x) * float(x) for x in g))
    got = optim.scalars_np(*tables[0], 0, [], "adam")["total_norm"]
    assert ulps(got, np.float32(exact)) <= 1


BAD_N = 2 * C + 1                                                          # the last chunk holds one element


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first", "last_alone_in_its_chunk", "last_of_the_first_chunk"])
@pytest.mark.parametrize("value", [np.nan, np.inf])
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_with_the_scaler_a_non_finite_gradient_skips_the_step(torch_cuda, kind, value, where):
    n, pos = BAD_N, {"first": 0, "last_alone_in_its_chunk": BAD_N - 1, "last_of_the_first_chunk": C - 1}[where]
    groups = two_groups(kind, [C + 2, n])
    p, g, m, v = tensors(n, 5, 1)
    g = g * np.float32(64.0)
    bad = g.copy()
    bad[pos] = value
    state = dict(SCALER, scale=np.float32(64.0), tracker=1)
    run = DeviceRun(torch_cuda, kind, p, m, v, groups, 7, state)
    cur = dict(p=p, m=m, v=v, step=7)
    seen = []
    for k, grads in enumerate((bad, g, g, g, bad)):                        # five launches in a row: both slots of both states
        got = run.run(grads, max_norm=1.0)
        want = optim.step_np(kind, cur["p"], grads, cur["m"], cur["v"], groups, cur["step"], max_norm=1.0, scaler=state, norm=got["table"])
        assert_equals_form(got, want, f"launch {k}")
        if grads is bad:
            assert got["found_inf"] and got["step"] == cur["step"] and got["tracker"] == 0 and got["scale"] == state["scale"] / 2
            for name in ("p", "m") + (() if kind == "sgd" else ("v",)):
                assert bits(got[name]).tobytes() == bits(cur[name]).tobytes(), f"launch {k}: {name} changed in a skipped step"
        cur = dict(p=want["p"], m=want["m"], v=want["v"], step=want["step"])
        state = dict(state, scale=want["scale"], tracker=want["tracker"])
        seen.append((float(got["scale"]), got["tracker"], got["step"]))
    assert seen == [(32.0, 0, 7), (32.0, 1, 8), (64.0, 0, 9), (64.0, 1, 10), (32.0, 0, 10)]


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first", "last_alone_in_its_chunk"])
@pytest.mark.parametrize("value", [np.nan, np.inf])
@pytest.mark.parametrize("kind", KINDS)
def test_without_the_scaler_a_non_finite_gradient_does_what_torch_does(torch_cuda, kind, value, where):
    import torch
    n, pos = BAD_N, {"first": 0, "last_alone_in_its_chunk": BAD_N - 1}[where]
    hyper = dict(HYPER[kind], weight_decay=0.0)                           # without decay a zero gradient leaves p as it is, in any rounding order
    p, g, _, _ = tensors(n, 9, 0)
    g[pos] = value
    run = DeviceRun(torch_cuda, kind, p, np.zeros_like(p), np.zeros_like(p), [dict(hyper, end=n)])
    got = run.run(g, max_norm=1.0)
    t = torch.nn.Parameter(torch.from_numpy(p.copy()))
    t.grad = torch.from_numpy(g.copy())
    torch.nn.utils.clip_grad_norm_([t], 1.0)
    {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "sgd": torch.optim.SGD}[kind]([t], **hyper).step()
    want = t.detach().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got["p"]), nan) and nan.sum() == (n if np.isnan(value) else 1)
    assert bits(got["p"][~nan]).tobytes() == bits(want[~nan]).tobytes()
    assert got["step"] == 1 and got["found_inf"]


def scene_optimizer(torch, name, **kw):
    sc = optim.SCENES[name]
    params = [torch.nn.Parameter(torch.from_numpy(a).cuda()) for a in optim.scene_params(sc["seed"])]
    groups = [dict(g, params=[p for p, k in zip(params, optim.SCENE_GROUP_OF) if k == i]) for i, g in enumerate(sc["groups"])]
    return getattr(optim, {"adam": "Adam", "adamw": "AdamW", "sgd": "SGD"}[sc["kind"]])(groups, max_norm=optim.SCENE_MAX_NORM, **kw), params


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(optim.SCENES))
@pytest.mark.parametrize("with_scaler", [False, True], ids=["plain", "scaler"])
def test_the_public_classes_run_the_fixtures_scenes(torch_cuda, name, with_scaler):
    torch = torch_cuda
    gold = load_golden("optim_scenes")
    key = name + ("_scaler" if with_scaler else "")
    opt, params = scene_optimizer(torch, name, zero_grads=True)
    a, sc = opt.arena, optim.SCENES[name]
    assert (a.offsets, a.ends, a.n) == optim.scene_layout()
    scaler = optim.LossScaler("cuda", **optim.SCALER) if with_scaler else None
    for k in range(optim.SCENE_STEPS):
        g = optim.flatten(optim.scene_grads(sc["seed"], k))
        if with_scaler:
            g = g * np.float32(scaler.get_scale())
            if k in optim.OVERFLOW_STEPS:
                g[a.n // 2] = np.inf
        assert not a.grad.any()                                            # zero_grads: the step cleared them
        for i, p in enumerate(params):
            p.grad.add_(a.views(torch.from_numpy(g).cuda(), i))            # what backward() does: accumulate into the views
        opt.step(scaler=scaler)
    mine, schedule = optim.run_scene_np(name, with_scaler)
    got = optim.unflatten(a.flat.cpu().numpy())
    assert bits(got).tobytes() == bits(mine).tobytes()                    # bit for bit the NumPy form
    e32 = float(gold[key + "_e32"][0])
    assert float(np.abs(got.astype(np.float64) - gold[key + "_p64"]).max()) <= 2 * e32
    skipped = len(optim.OVERFLOW_STEPS) if with_scaler else 0
    assert opt.step_count() == optim.SCENE_STEPS - skipped
    if with_scaler:
        assert (scaler.get_scale(), scaler.state_dict()["_growth_tracker"]) == schedule[-1]
    sd = opt.state_dict()
    assert len(sd["state"]) == 4 and (name == "sgd" or float(sd["state"][0]["step"]) == optim.SCENE_STEPS - skipped)


@pytest.mark.gpu
def test_three_steps_of_a_two_conv_module_end_to_end(torch_cuda):
    torch = torch_cuda
    gold = load_golden("optim_scenes")
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(8, 2, 1))
    init, o = gold["e2e_init"], 0
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.from_numpy(init[o:o + p.numel()]).view(p.shape))
            o += p.numel()
    net = net.cuda()
    opt = optim.AdamW(net.parameters(), max_norm=optim.SCENE_MAX_NORM, **optim.E2E["groups"][0])
    x = torch.from_numpy(gold["e2e_x"]).cuda()
    before = net(x).detach().clone()
    for _ in range(optim.E2E["steps"]):
        opt.zero_grad()
        (net(x).square().mean() * optim.E2E["loss_gain"]).backward()
        opt.step()
    a = opt.arena
    got = np.concatenate([a.views(a.flat, i).detach().cpu().numpy().reshape(-1) for i in range(len(a.params))])
    err, e32 = float(np.abs(got.astype(np.float64) - gold["e2e_p64"]).max()), float(gold["e2e_e32"][0])
    print(f"e2e: err {err:.3e}  e32 {e32:.3e}  total_norm {opt.total_norm():.4f}")
    assert err <= 2 * e32
    assert opt.step_count() == optim.E2E["steps"] and opt.total_norm() > 0
    # the module's forward uses the updated views
    F = torch.nn.functional
    after = net(x)
    by_hand = F.conv2d(F.relu(F.conv2d(x, a.views(a.flat, 0), a.views(a.flat, 1), padding=1)), a.views(a.flat, 2), a.views(a.flat, 3))
    assert torch.equal(after, by_hand) and not torch.equal(after, before)
    assert all(p.data_ptr() == a.flat.data_ptr() + 4 * off for p, off in zip(net.parameters(), a.offsets))
