"""Guard-band tests of the eighth binding table (include/unetpp_loss_grad.h): both launching entries with every tensor
between random guard bytes (tests/guarded.py), at every alignment phase the kernels distinguish, with the assertions of
tests/test_gpu_guarded.py: guards intact, equal to the NumPy form bit for bit, the same bits with the filling complemented
(so nothing outside the tensors reaches the result and every output byte is written), inputs unchanged.
  loss_grad: logits 0..3 elements off a 16-byte boundary, the gradient 0..3 elements off independently (all 16 pairs), the
             target 0..3 bytes off, coefficients and scale one element off; ragged sizes; the in-place form.
  narrow_target: the int64 source at both 8-byte phases, the uint8 destination at 0..15.
Run on the GPU box:  python -m pytest tests/test_gpu_guarded_loss_grad.py -m gpu"""
import numpy as np
import pytest

import guarded
import test_gpu_guarded as tg
from test_gpu_guarded import model, torch_cuda  # noqa: F401  (fixtures)
from unet_amd import loss as ls
from unet_amd import loss_grad as lg

COVERED = {"unetpp_loss_grad_f32": "test_loss_grad, test_loss_grad_in_place", "unetpp_loss_narrow_target_i64": "test_narrow_target"}
# Symbols of the eighth table that write no caller-provided device buffer.
EXCLUDED_LOSS_GRAD = {"unetpp_loss_grad_layout": "layout query"}

# (logits offset, gradient offset) in elements, every pair; the target's byte offset runs through 0..3 along them
GRAD_OFFSETS = [(lo, go, (lo + 2 * go + 1) % 4) for lo in range(4) for go in range(4)]
# ragged sizes of tests/test_gpu_loss_grad.py: odd C H W (frames at different pads), a span plus 64, seven classes
GRAD_SHAPES = [(2, 3, 17, 23), (1, 3, 65, 64), (3, 7, 33, 57)]
NARROW_OFFSETS = [(8 * (d % 2), d) for d in range(16)] + [(8 * ((d + 1) % 2), d) for d in (0, 5, 10, 15)]
NARROW_SIZES = (1, 15, 33, 782, 4096 + 17)


def scene(shape, gamma):
    B, C, H, W = shape
    logits, target = ls.make_logits(B, C, H, W, 70 + C, "nonfinite"), ls.make_target(B, C, H, W, 70 + C, "out_of_range")
    table, _ = ls.loss_sums_np(logits, target, gamma)
    cw = ls.scene_class_weights(C)
    coef = (lg.coefficients_from_sums(table, H * W, "combined", class_weights=cw, dice_ignore_bg=False) +
            lg.coefficients_from_sums(table, H * W, "advanced", class_weights=cw, focal_gamma=gamma))
    return logits, target, coef


def run_grad(torch, model, shape, lo, go, to, in_place=False):
    from unet_amd import _lib
    gamma, scale = 2, np.float32([-0.75])
    logits, target, coef = scene(shape, gamma)
    want = lg.loss_grad_np(logits, target, coef, gamma, scale[0])
    seen = {}

    def run(g):
        t = {"logits": g.place(logits, 4 * lo, "logits"), "target": g.place(target, to, "target"), "coef": g.place(coef, 4, "coef"),
             "scale": g.place(scale, 4, "scale")}
        with g.allocations(models=[model], lib_module=_lib):
            out = lg.loss_grad(model, t["logits"], t["target"], t["coef"], gamma, t["scale"], out=t["logits"] if in_place else None)
            torch.cuda.synchronize()
        seen["symbols"] = set(g.symbols) - set(tg.EXCLUDED)
        assert out.data_ptr() % 16 == 4 * (lo if in_place else go)
        for k, a in (("target", target), ("coef", coef), ("scale", scale)) + (() if in_place else (("logits", logits),)):
            assert t[k].cpu().numpy().tobytes() == a.tobytes(), f"input {k!r} was written"
        return out

    got = guarded.two_fillings(torch, run, seed=lo + 4 * go, align=lambda s, dtype, ctx: 4 * go if len(s) == 4 and dtype == torch.float32 else None)
    assert seen["symbols"] == {"unetpp_loss_grad_f32"}
    (_, dtype, shp, raw), = got
    assert dtype == "float32" and tuple(shp) == shape
    assert np.array_equal(raw.view(np.uint32), np.ascontiguousarray(want).view(np.uint32).reshape(-1))
    return raw


@pytest.mark.gpu
@pytest.mark.parametrize("lo,go,to", GRAD_OFFSETS)
@pytest.mark.parametrize("shape", GRAD_SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_loss_grad(torch_cuda, model, shape, lo, go, to):  # noqa: F811
    run_grad(torch_cuda, model, shape, lo, go, to)


@pytest.mark.gpu
@pytest.mark.parametrize("lo,go,to", [(0, 0, 0), (1, 2, 3), (3, 1, 2), (2, 3, 1)])
def test_loss_grad_seven_classes(torch_cuda, model, lo, go, to):  # noqa: F811
    run_grad(torch_cuda, model, GRAD_SHAPES[2], lo, go, to)


@pytest.mark.gpu
@pytest.mark.parametrize("lo", range(4))
def test_loss_grad_in_place(torch_cuda, model, lo):  # noqa: F811
    """out = logits at each phase: the same bits as the out-of-place form."""
    a = run_grad(torch_cuda, model, GRAD_SHAPES[0], lo, lo, (lo + 1) % 4, in_place=True)
    assert np.array_equal(a, run_grad(torch_cuda, model, GRAD_SHAPES[0], lo, (lo + 1) % 4, lo))


@pytest.mark.gpu
@pytest.mark.parametrize("src_off,dst_off", NARROW_OFFSETS)
def test_narrow_target(torch_cuda, model, src_off, dst_off):  # noqa: F811
    from unet_amd import _lib
    torch = torch_cuda
    r = np.random.default_rng(16 * src_off + dst_off)
    for n in NARROW_SIZES:
        t = r.integers(0, 255, n).astype(np.int64)
        t[r.permutation(n)[:max(1, n // 7)]] = np.resize(np.int64([-100, 255, 256, -1, 2 ** 40]), max(1, n // 7))
        want = np.where((t >= 0) & (t <= 254), t, 255).astype(np.uint8)
        seen = {}

        def run(g):
            src = g.place(t, src_off, "target_i64")
            with g.allocations(models=[model], lib_module=_lib):
                out = lg.narrow_target(model, src)
                torch.cuda.synchronize()
            seen["symbols"] = set(g.symbols) - set(tg.EXCLUDED)
            assert out.data_ptr() % 16 == dst_off and src.data_ptr() % 16 == src_off
            assert src.cpu().numpy().tobytes() == t.tobytes()
            return out

        (_, dtype, shp, raw), = guarded.two_fillings(torch, run, seed=n, u8_out_offset=dst_off)
        assert seen["symbols"] == {"unetpp_loss_narrow_target_i64"} and dtype == "uint8" and np.array_equal(raw, want), n
