"""The optimiser step's NumPy form and public interface (unet_amd/optim.py), without a GPU.

  distance to torch   step_np after SCENE_STEPS steps against torch's float64 CPU result of the fixture
                      (tests/golden/optim_scenes.npz, scripts/make_golden_optim.py): eform <= 2 * e32 per scene, e32 torch-float32's
                      own distance.  The factor 2 is not derived: both are float32 chains of equal length in different rounding order.
  norm                grad_norm_np against math.fsum of the exact float64 squares, rounded once: the float32 norm within 1 ulp.
                      Derived: float64 accumulation of n <= 2^27 exact terms errs by < n * 2^-53 relative, far below 2^-24.
  scaler              the (scale, tracker) schedule equals the recorded one with ==, two overflows, growth_interval = 2
  interfaces          state_dict round trips through torch.optim on the CPU; torch's four schedulers drive the param groups;
                      ParamArena's layout; the refusal of set_to_none=True and of a detached p.grad"""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from unet_amd import optim

GOLD = load_golden("optim_scenes")
KEYS = [name + suffix for name in optim.SCENES for suffix in ("", "_scaler")]


@pytest.mark.parametrize("key", KEYS)
def test_step_np_is_as_close_to_torch_float64_as_torch_float32(key):
    name, scaler = key.split("_")[0], key.endswith("_scaler")
    mine, schedule = optim.run_scene_np(name, scaler)
    p64, e32 = GOLD[key + "_p64"], float(GOLD[key + "_e32"][0])
    eform = float(np.abs(mine.astype(np.float64) - p64).max())
    print(f"{key}: eform {eform:.3e}  e32 {e32:.3e}")
    assert eform <= 2 * e32
    if scaler:
        assert [(s, float(t)) for s, t in schedule] == [tuple(r) for r in GOLD[key + "_sched"].tolist()]


def test_the_scaler_schedule_has_two_backoffs_and_grows_every_second_clean_step():
    sched = GOLD["adamw_scaler_sched"]
    scale, tracker, want = np.float32(optim.SCALER["init_scale"]), 0, []
    for k in range(optim.SCENE_STEPS):
        scale, tracker = optim.scaler_update_np(scale, tracker, k in optim.OVERFLOW_STEPS, optim.SCALER["growth_factor"],
                                                optim.SCALER["backoff_factor"], optim.SCALER["growth_interval"])
        want.append((float(scale), float(tracker)))
    assert want == [tuple(r) for r in sched.tolist()]
    halved = [k for k in range(1, optim.SCENE_STEPS) if sched[k, 0] < sched[k - 1, 0]]
    assert halved == list(optim.OVERFLOW_STEPS) and all(sched[k, 1] == 0 for k in halved)
    # a scale that would overflow is kept (torch's rule), the tracker restarts
    big = np.float32(2.0 ** 127)
    assert optim.scaler_update_np(big, 1, False, 2.0, 0.5, 2) == (big, 0)


def ulps(a, b):
    a, b = (int(np.float32(x).view(np.int32)) for x in (a, b))
    return abs(a - b)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, optim.GRANULE - 1, optim.GRANULE, optim.GRANULE + 1, 3 * optim.GRANULE + 7])
def test_grad_norm_np_is_within_one_ulp_of_the_exact_norm(n):
    rng = np.random.default_rng(n)
    g = (rng.standard_normal(n) * np.exp(rng.uniform(-30, 10, n))).astype(np.float32)
    partial, flag = optim.grad_norm_np(g)
    assert partial.shape == flag.shape == (optim.parts_for(n),) and not flag.any()
    exact = math.sqrt(math.fsum(float(x) * float(x) for x in g))          # each square is exact in float64
    got = optim.scalars_np(partial, flag, 0, [], "adam")["total_norm"]
    assert got.dtype == np.float32 and ulps(got, np.float32(exact)) <= 1


def test_grad_norm_np_flags_the_chunk_that_holds_a_non_finite_element():
    g = np.ones(2 * optim.GRANULE + 5, np.float32)
    g[-1] = np.nan
    assert optim.grad_norm_np(g)[1].tolist() == [0, 0, 1]
    g[-1], g[0] = 1, np.inf
    assert optim.grad_norm_np(g)[1].tolist() == [1, 0, 0]


def test_chunks_follow_from_n_alone():
    assert optim.chunk_for(1) == optim.chunk_for(optim.GRANULE * optim.MAX_PARTIALS) == optim.GRANULE
    assert optim.chunk_for(optim.GRANULE * optim.MAX_PARTIALS + 1) == 2 * optim.GRANULE
    assert optim.parts_for(optim.MAX_N) <= optim.MAX_PARTIALS and optim.chunk_for(optim.MAX_N) % (4 * optim.THREADS) == 0


def test_pow_np_is_square_and_multiply():
    sq = 0.9 * 0.9
    assert optim.pow_np(0.9, 0) == 1.0 and optim.pow_np(0.9, 1) == 0.9 and optim.pow_np(0.9, 2) == sq
    assert optim.pow_np(0.9, 5) == 0.9 * (sq * sq) and optim.pow_np(0.9, 6) == sq * (sq * sq)
    assert abs(optim.pow_np(0.999, 1000) - 0.999 ** 1000) <= 1e-13


def test_without_a_scaler_a_non_finite_norm_flows_through_the_arithmetic():
    groups = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, end=8)]
    g = np.float32([1, 2, 3, np.inf, 0, -1, 0.5, 4])
    out = optim.step_np("adam", np.ones(8, np.float32), g, np.zeros(8, np.float32), np.zeros(8, np.float32), groups, 0, max_norm=1.0)
    # coef = 1 / inf = 0: the infinite element becomes 0 * inf = NaN, every other gradient 0 and its parameter stays, as in torch
    assert out["total_norm"] == np.inf and np.isnan(out["p"]).tolist() == [k == 3 for k in range(8)] and out["step"] == 1
    t = torch.nn.Parameter(torch.ones(8))
    t.grad = torch.from_numpy(g.copy())
    torch.nn.utils.clip_grad_norm_([t], 1.0)
    torch.optim.Adam([t], lr=1e-3).step()
    assert np.array_equal(np.isnan(t.detach().numpy()), np.isnan(out["p"]))


def small_net():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3), torch.nn.ReLU(), torch.nn.Conv2d(5, 2, 1))


def test_param_arena_holds_parameters_and_gradients_in_one_flat_buffer():
    net, ref = small_net(), small_net()
    arena = optim.ParamArena([{"params": list(net[0].parameters())}, {"params": list(net[2].parameters())}])
    assert arena.offsets == [0, 136, 144, 156] and arena.ends == [144, 160] and arena.n == 160
    x = torch.randn(2, 3, 8, 8)
    assert torch.equal(net(x), ref(x))                                    # the views hold the values
    net(x).square().sum().backward()
    ref(x).square().sum().backward()
    arena.check()
    flat = arena.grad.numpy()
    for i, (p, q, o) in enumerate(zip(net.parameters(), ref.parameters(), arena.offsets)):
        assert (arena.grad.data_ptr() + 4 * o) % 16 == 0 and p.grad.data_ptr() == arena.grad.data_ptr() + 4 * o
        assert np.array_equal(flat[o:o + p.numel()], q.grad.numpy().reshape(-1))
        assert p.data_ptr() == arena.flat.data_ptr() + 4 * o
    pad = np.ones(160, bool)
    for p, o in zip(arena.params, arena.offsets):
        pad[o:o + p.numel()] = False
    assert pad.sum() == 160 - 135 - 5 - 10 - 2 and not flat[pad].any() and not arena.flat.numpy()[pad].any()
    net(x).square().sum().backward()                                       # autograd accumulates in place
    assert np.array_equal(arena.grad.numpy()[:135], 2 * ref[0].weight.grad.numpy().reshape(-1))
    arena.zero_grad()
    assert not arena.grad.any() and net[0].weight.grad.data_ptr() == arena.grad.data_ptr()


def test_set_to_none_and_a_detached_grad_are_refused():
    net = small_net()
    opt = optim.AdamW(net.parameters(), lr=1e-3)
    with pytest.raises(RuntimeError, match="set_to_none=True"):
        opt.zero_grad(set_to_none=True)
    opt.zero_grad()
    opt.arena.check()
    net.zero_grad(set_to_none=True)                                        # what torch's default does
    with pytest.raises(RuntimeError, match="set_to_none=True"):
        opt.arena.check()
    net2 = small_net()
    arena = optim.ParamArena(net2.parameters())
    net2[0].bias.grad = torch.zeros(5)
    with pytest.raises(RuntimeError, match="set_to_none=True"):
        arena.check()


def test_step_on_a_cpu_arena_is_an_error_not_a_fallback():
    opt = optim.SGD(small_net().parameters(), lr=0.1, momentum=0.9)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()


def test_more_than_eight_groups_and_other_dtypes_are_refused():
    with pytest.raises(ValueError, match="at most 8"):
        optim.ParamArena([{"params": [torch.nn.Parameter(torch.zeros(2))]} for _ in range(9)])
    with pytest.raises(TypeError, match="float32"):
        optim.ParamArena([torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))])
    with pytest.raises(ValueError, match="not supported"):
        optim.Adam(small_net().parameters(), amsgrad=True)


@pytest.mark.parametrize("name,torch_cls,kw", [("AdamW", torch.optim.AdamW, dict(lr=2e-3, betas=(0.8, 0.9), weight_decay=0.05)),
                                               ("Adam", torch.optim.Adam, dict(lr=1e-3)),
                                               ("SGD", torch.optim.SGD, dict(lr=0.1, momentum=0.9))])
def test_state_dict_round_trips_through_torch(name, torch_cls, kw):
    ref = small_net()
    topt = torch_cls(ref.parameters(), **kw)
    for k in range(3):
        for p in ref.parameters():
            p.grad = torch.full_like(p, 0.1 * (k + 1))
        topt.step()
    sd = topt.state_dict()
    net = small_net()
    opt = getattr(optim, name)(net.parameters(), **kw)
    assert opt.state_dict()["state"] == {}                                  # nothing before the first step, as in torch
    opt.load_state_dict(sd)                                                 # a checkpoint written by a reference loop resumes here
    a = opt.arena
    for i, p in enumerate(ref.parameters()):
        st = topt.state[p]
        assert torch.equal(a.views(a.m, i), st["momentum_buffer" if name == "SGD" else "exp_avg"])
        if name != "SGD":
            assert torch.equal(a.views(a.v, i), st["exp_avg_sq"])
    assert opt.step_count() == (1 if name == "SGD" else 3)
    back = opt.state_dict()
    assert back["param_groups"] == sd["param_groups"] and set(back["state"]) == set(sd["state"])
    for k, st in sd["state"].items():
        assert set(back["state"][k]) == set(st)
        for field, value in st.items():
            assert torch.equal(torch.as_tensor(back["state"][k][field]), torch.as_tensor(value)), (k, field)
    topt2 = torch_cls(small_net().parameters(), **kw)                       # and the other way round
    topt2.load_state_dict(back)
    for p in topt2.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    topt2.step()


SCHEDULERS = {
    "cosine": lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=7, eta_min=1e-6),
    "warm_restarts": lambda o: torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(o, T_0=3, T_mult=2, eta_min=1e-6),
    "step": lambda o: torch.optim.lr_scheduler.StepLR(o, step_size=2, gamma=0.5),
    "plateau": lambda o: torch.optim.lr_scheduler.ReduceLROnPlateau(o, mode="max", factor=0.5, patience=1),
}


@pytest.mark.parametrize("which", list(SCHEDULERS))
def test_torchs_schedulers_drive_the_param_groups(which):
    def groups(net):
        return [{"params": list(net[0].parameters())}, {"params": list(net[2].parameters()), "lr": 5e-3}]
    mine, theirs = optim.AdamW(groups(small_net()), lr=1e-3), torch.optim.AdamW(groups(small_net()), lr=1e-3)
    seq = []
    for o in (mine, theirs):
        sched, lrs = SCHEDULERS[which](o), []
        for epoch in range(10):
            o._opt_called = True                                            # the schedulers only warn about the call order
            sched.step(0.5 - 0.01 * epoch) if which == "plateau" else sched.step()
            lrs.append([g["lr"] for g in o.param_groups])
        seq.append(lrs)
    assert seq[0] == seq[1] and len({tuple(r) for r in seq[0]}) > 1
    assert optim.group_doubles(mine.param_groups[1], "adamw")[0] == seq[0][-1][1]      # what the next launch is given


def test_loss_scaler_on_the_cpu_scales_and_round_trips():
    s = optim.LossScaler("cpu", init_scale=1024.0, growth_interval=2)
    assert s.get_scale() == 1024.0 and float(s.scale(torch.tensor(0.5))) == 512.0
    sd = s.state_dict()
    assert sd == {"scale": 1024.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2, "_growth_tracker": 0}
    assert set(sd) == set(torch.amp.GradScaler("cpu").state_dict())
    s2 = optim.LossScaler("cpu")
    s2.load_state_dict(dict(sd, scale=8.0, _growth_tracker=1))
    assert s2.state_dict()["scale"] == 8.0 and s2.state_dict()["_growth_tracker"] == 1 and s2.growth_interval == 2
