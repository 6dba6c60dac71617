"""Guard-band tests of the optimiser library (include/optim/unetpp_optim.h): both launches with every tensor they touch (parameters,
gradients, both moments, the workspace, the optimiser's and the scaler's state) between random guard bytes, tests/guarded.py used
by hand (Guard.place, Guard.check, two_fillings; the library takes no engine, so there is no call hook to patch).  Asserted:
guards intact, the results bit for bit those of the NumPy form, the same bits with the filling complemented (nothing outside the
tensors reaches a result, every output element is written), and the words of the state buffers a launch does not own unchanged.
  float32 tensors at payload offsets 0 and 4 modulo 16 (all at 0: the 16-byte accesses; any at 4: the 4-byte accesses);
  the workspace at both 8-byte phases; the ragged sizes of tests/test_gpu_optim.py.
Run on the GPU box:  python -m pytest tests/test_gpu_guarded_optim.py -m gpu"""
import numpy as np
import pytest

import guarded
import test_gpu_optim as tg
from test_gpu_optim import torch_cuda  # noqa: F401  (fixture)
from unet_amd import optim

COVERED = {"unetpp_optim_grad_norm_f32": "test_both_launches_between_guards", "unetpp_optim_step_f32": "test_both_launches_between_guards"}
EXCLUDED_OPTIM = {"unetpp_optim_layout": "layout query", "unetpp_optim_workspace_bytes": "size query", "unetpp_optim_version": "version string"}

# payload offsets modulo 16 of (p, g, m, v, workspace, state, scaler state)
PHASES = {"all_16": (0, 0, 0, 0, 0, 0, 0), "all_4": (4, 4, 4, 4, 8, 4, 4), "g_4": (0, 4, 0, 0, 0, 4, 0), "m_4": (0, 0, 4, 0, 8, 0, 4),
          "p_v_4": (4, 0, 0, 4, 8, 4, 4)}
SIZES = tg.SIZES
MARK = 0x5A5A5A5A                                                          # fills the state words no launch owns


def run_case(torch, kind, n, phases, use_scaler, zero_grads, seed):
    step = (0, 1, 999)[seed % 3]
    groups = tg.two_groups(kind, [n // 2, n] if n >= 2 else [n])
    p, g, m, v = tg.tensors(n, seed, step)
    scaler = dict(tg.SCALER, scale=np.float32(256.0), tracker=1) if use_scaler else None
    if use_scaler:
        g = g * np.float32(256.0)
    offsets = dict(zip(("p", "g", "m", "v", "workspace", "state", "scaler_state"), phases))

    def run(guard):
        def place(a, what):
            if what in ("state", "scaler_state"):                          # the read slot as given, every other word marked
                a = a.copy()
                a[optim.SLOT_WORDS:] = MARK
                for k in range(optim.SLOT_WORDS):
                    if k not in ((optim.ST_STEP,) if what == "state" else (optim.ST_SCALE, optim.ST_TRACKER)):
                        a[k] = MARK
            if what == "workspace":                                        # launch A writes the whole table: start from noise
                a = guard.rng.random(a.size)
            return guard.place(a, offsets[what], what)
        dev = tg.DeviceRun(torch, kind, p, m, v, groups, step, scaler, place)
        got = dev.run(g, max_norm=1.0, zero_grads=zero_grads)
        for name, t, own in (("state", dev.state, (optim.ST_STEP, optim.ST_NORM, optim.ST_FOUND_INF)),
                             ("scaler_state", dev.scaler_state, (optim.ST_SCALE, optim.ST_TRACKER))):
            if t is not None:
                words = t.cpu().numpy().view(np.uint32)
                kept = [k for k in range(2 * optim.SLOT_WORDS) if k % optim.SLOT_WORDS not in own]
                assert (words[kept] == MARK).all(), f"{name}: a word the launch does not own was written"
        return {k: got[k] for k in ("p", "g", "m", "v", "step", "found_inf", "scale", "tracker") if got[k] is not None} | {
            "total_norm": np.float32([got["total_norm"]]), "partial": got["table"][0], "flag": got["table"][1]}

    res = dict((path, raw) for path, _, _, raw in guarded.two_fillings(torch, run, seed=seed))
    partial, flag = res["result['partial']"].view(np.float64), res["result['flag']"].view(np.uint32)
    want = optim.step_np(kind, p, g, m, v, groups, step, max_norm=1.0, scaler=scaler, zero_grads=zero_grads, norm=(partial, flag))
    ref = optim.grad_norm_np(g)
    assert partial.tobytes() == ref[0].tobytes() and flag.tobytes() == ref[1].tobytes()
    for k in ("p", "g", "m") + (() if kind == "sgd" else ("v",)):
        assert res[f"result[{k!r}]"].tobytes() == tg.bits(want[k]).tobytes(), k
    assert res["result['total_norm']"].tobytes() == np.float32(want["total_norm"]).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("phase", list(PHASES))
def test_both_launches_between_guards(torch_cuda, phase, n):  # noqa: F811
    i = list(PHASES).index(phase) + SIZES.index(n)
    run_case(torch_cuda, tg.KINDS[i % 3], n, PHASES[phase], use_scaler=bool(i % 2), zero_grads=bool((i // 2) % 2), seed=n + i)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", tg.KINDS)
def test_a_skipped_step_between_guards(torch_cuda, kind):  # noqa: F811
    """With the scaler and a non-finite gradient nothing but the gradients (zero_grads) and the two states may be written."""
    n = optim.GRANULE + 5
    groups = tg.two_groups(kind, [n])
    p, g, m, v = tg.tensors(n, 3, 1)
    g[n - 1] = np.inf
    scaler = dict(tg.SCALER, scale=np.float32(2.0), tracker=1)

    def run(guard):
        dev = tg.DeviceRun(torch_cuda, kind, p, m, v, groups, 4, scaler, lambda a, what: guard.place(a, 4 if what in ("g", "m") else 0, what))
        got = dev.run(g, max_norm=1.0, zero_grads=True)
        return {k: got[k] for k in ("p", "g", "m", "step", "scale", "tracker")}

    res = dict((path, raw) for path, _, _, raw in guarded.two_fillings(torch_cuda, run, seed=1))
    assert res["result['p']"].tobytes() == p.tobytes() and res["result['m']"].tobytes() == m.tobytes() and not res["result['g']"].any()
