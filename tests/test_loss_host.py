"""The NumPy form of the validation-loss sums and the float64 algebra on their table (unet_amd/loss.py) against the
reference's own losses (tests/golden/loss_scenes.npz, scripts/make_golden_loss.py), what is particular to include/unetpp_loss.h,
and the argument checks that need no device.  No GPU.

The bar: every loss from loss_sums_np + the algebra lies no further from the reference's float64 run than the reference's
own float32 run does (d32, the maximum over the scenes, per loss).  As measured when the fixture was made
(tests/golden/README_loss.txt): d32 between 1.2e-7 (cross-entropy) and 9.5e-7 (Tversky), the form's own distance between
6.6e-9 and 2.9e-8."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from unet_amd import _lib
from unet_amd import loss as ls

README = os.path.join(ROOT, "tests", "golden", "README_loss.txt")


@pytest.fixture(scope="module")
def golden():
    g = load_golden("loss_scenes")
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def facts(golden):
    return ls.fixture_facts(golden)


# ---- exp32 and log32 ------------------------------------------------------------------------------------------------------------
def test_primitive_accuracy(golden):
    """At most 1 float32 ulp from float64 np.exp on [-87, 0] and np.log on [1, 8], on a dense sample; the measured maxima
    are the ones README_loss.txt records."""
    d = np.linspace(-87.0, 0.0, 2_000_001).astype(np.float32)
    s = np.linspace(1.0, 8.0, 2_000_001).astype(np.float32)
    e_ulp = ls.ulp_error(ls.exp32_np(d), np.exp(d.astype(np.float64)))
    l_ulp = ls.ulp_error(ls.log32_np(s[1:]), np.log(s[1:].astype(np.float64)))
    print(f"exp32_np: {e_ulp:.3f} ulp on [-87, 0]; log32_np: {l_ulp:.3f} ulp on (1, 8]")
    assert e_ulp <= 1.0 and l_ulp <= 1.0
    # float64 np.exp / np.log may differ in their last bit between builds of NumPy: that moves these figures by 1e-9
    assert abs(e_ulp - float(golden["exp32_ulp"])) < 1e-6 and abs(l_ulp - float(golden["log32_ulp"])) < 1e-6
    with open(README) as f:
        text = f.read()
    assert f"largest error {float(golden['exp32_ulp']):.3f} float32 ulps against float64 np.exp" in text
    assert f"largest error {float(golden['log32_ulp']):.3f} float32 ulps against float64 np.log" in text


def test_primitive_fixed_points():
    assert ls.exp32_np(np.float32(0.0)) == 1.0 and ls.exp32_np(np.float32(-0.0)) == 1.0 and ls.log32_np(np.float32(1.0)) == 0.0
    below = np.float32([-87.00001, -88, -1000, -3e38, -np.inf])
    assert (ls.exp32_np(below) == 0).all() and ls.exp32_np(np.float32(-87.0)) > np.finfo(np.float32).tiny
    assert ls.exp32_np(below).dtype == np.float32 and ls.log32_np(np.float32([2.0])).dtype == np.float32
    assert abs(float(ls.log32_np(np.float32(8.0))) - np.log(8.0)) < 3e-7


# ---- the table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", [s[0] for s in ls.LOSS_SCENES if s[4] <= 80])
def test_table_invariants(scene):
    """T over the classes plus the two outside counters is H W; P sums to one per pixel of the sums within the flooring
    (each of the C terms loses less than 2^-32, a quotient's rounding at most 2^-24 relative); I <= P; a frame's row does
    not depend on the batch it is in."""
    logits, target = ls.make_scene(scene)
    B, C, H, W = logits.shape
    table, outside = ls.loss_sums_np(logits, target)
    assert table.dtype == np.uint64 and table.shape == (B, C, 5) and outside.dtype == np.uint32 and outside.shape == (B, 2)
    T = table[:, :, 0].astype(np.int64)
    assert (T.sum(1) + outside.astype(np.int64).sum(1) == H * W).all()
    n = T.sum(1).astype(np.float64)
    p_total = table[:, :, 1].astype(np.float64).sum(1) / ls.P_SCALE
    assert (p_total <= n * (1 + C * 2.0 ** -23)).all() and (p_total >= n * (1 - C * 2.0 ** -23) - n * C * 2.0 ** -32).all()
    assert (table[:, :, 2] <= table[:, :, 1]).all() and (table[:, :, 4] <= table[:, :, 3]).all()      # (1 - p)^2 <= 1
    for b in range(B):
        one = ls.loss_sums_np(logits[b:b + 1], target[b:b + 1])
        assert np.array_equal(one[0][0], table[b]) and np.array_equal(one[1][0], outside[b])
    rev = ls.loss_sums_np(logits[::-1].copy(), target[::-1].copy())
    assert np.array_equal(rev[0][::-1], table) and np.array_equal(rev[1][::-1], outside)


def test_gamma_and_the_clamp():
    logits, target = ls.make_scene("plain3")
    t0, t1, t2, t4 = (ls.loss_sums_np(logits, target, g)[0] for g in (0, 1, 2, 4))
    assert np.array_equal(t0[:, :, 4], t0[:, :, 3])                                   # gamma 0: FOC is NLL
    assert np.array_equal(t0[:, :, :4], t2[:, :, :4]) and (t1[:, :, 4] >= t2[:, :, 4]).all() and (t2[:, :, 4] >= t4[:, :, 4]).all()
    # a target class 3e38 below the maximum: d = -inf, p = 0, nll = +inf, clamped to 131072 in both columns
    x = np.zeros((1, 2, 1, 2), np.float32)
    x[0, 0, 0, 0], x[0, 1, 0, 0] = -3e38, 3e38
    table, outside = ls.loss_sums_np(x, np.uint8([[[0, 1]]]))
    assert not outside.any() and table[0, 0].tolist() == [1, 2 ** 31, 0, 2 ** 41, 2 ** 41]
    assert table[0, 1, 0] == 1 and table[0, 1, 1] == 2 ** 32 + 2 ** 31 and table[0, 1, 2] == 2 ** 31
    assert table[0, 1, 3] == round(float(ls.log32_np(np.float32(2.0))) * 2 ** 24)


def test_special_pixels_stay_out():
    """A pixel with target >= C or a non-finite logit changes nothing but its counter: the table equals that of the scene
    with those pixels' T removed."""
    logits, target = ls.make_scene("both3")
    table, outside = ls.loss_sums_np(logits, target)
    assert outside[:, 0].all() and outside[:, 1].any()
    p, nll, foc, t, kind = ls.pixel_terms_np(logits, target)
    assert np.array_equal(np.stack([(kind == 1).sum(1), (kind == 2).sum(1)], 1), outside)
    clean_logits = np.where((kind != 0).reshape(target.shape)[:, None], np.float32(0), logits)
    clean_target = np.where((kind != 0).reshape(target.shape), np.uint8(0), target)
    full, none = ls.loss_sums_np(clean_logits, clean_target)
    assert not none.any()
    extra = (kind != 0).sum(1)                                  # the cleaned pixels: logits 0, target 0
    assert np.array_equal(full[:, 1:, [0, 2, 3, 4]], table[:, 1:, [0, 2, 3, 4]])
    assert np.array_equal(full[:, 0, 0] - extra.astype(np.uint64), table[:, 0, 0])
    with pytest.raises(ValueError, match="frame 0"):
        ls._raise_outside(outside, 3)


# ---- the bar --------------------------------------------------------------------------------------------------------------------
def test_losses_within_the_references_own_float32_noise(golden, facts):
    d32 = {k: float(v) for k, v in zip(ls.LOSSES, golden["d32"])}
    for k in ls.LOSSES:
        print(f"{k}: form {facts['dist'][k]:.3e} at {facts['worst'][k]}, d32 {d32[k]:.3e}")
    assert all(facts["dist"][k] <= d32[k] for k in ls.LOSSES), (facts["dist"], d32)
    # the recorded distances are these ones
    assert np.allclose([facts["dist"][k] for k in ls.LOSSES], golden["form"], rtol=1e-3, atol=0)
    with open(README) as f:
        text = f.read()
    for k, loss in enumerate(ls.LOSSES):
        assert re.search(rf"^  {loss}\s+{float(golden['d32'][k]):.3e} .*{float(golden['form'][k]):.3e}", text, re.M), loss


def test_fixture_branches(golden, facts):
    """The Dice fallback, skip_empty on a single frame, a class absent from one frame only, exp32's underflow, the weighted
    and the unweighted means and all three kinds of special scene are met (fixture_facts asserts it); the compared scenes
    are the ones without special pixels, and the reference's float32 run of every one is stored beside its float64 run."""
    assert {"dice_fallback", "skip_empty_single_frame", ("weighted", True), ("weighted", False)} <= facts["branches"]
    compared = [s[0] for s in ls.LOSS_SCENES if s[6] not in ls.SPECIAL and s[7] not in ls.SPECIAL]
    assert len(compared) >= 8 and all(golden[f"{n}_ref64"].shape == golden[f"{n}_ref32"].shape == (len(ls.PARAM_SETS), len(ls.LOSSES)) for n in compared)


def test_algebra_by_hand():
    """One frame, two classes, round numbers: every expression of the reference on a table written by hand."""
    T, P, I = [6, 2], [5.5, 2.5], [5.0, 1.0]
    NLL, FOC = [1.5, 3.0], [0.5, 2.0]
    table = np.array([[[T[c], int(P[c] * 2 ** 32), int(I[c] * 2 ** 32), int(NLL[c] * 2 ** 24), int(FOC[c] * 2 ** 24)] for c in range(2)]], np.uint64)
    assert ls.cross_entropy_from_sums(table) == 4.5 / 8 and ls.cross_entropy_from_sums(table, [1.0, 3.0]) == (1.5 + 9.0) / (6 + 6)
    d0, d1 = (10 + 1e-5) / (11.5 + 1e-5), (2 + 1e-5) / (4.5 + 1e-5)
    assert ls.dice_from_sums(table) == 1 - d1
    assert ls.dice_from_sums(table, ignore_bg=False) == 1 - np.array([d0, d1]).mean()
    assert ls.dice_from_sums(table, ignore_bg=False, class_weights=[1.0, 3.0]) == 1 - (d0 + 3 * d1) / (4 + 1e-6)
    assert ls.focal_from_sums(table, 8) == 2.5 / 8 and ls.focal_from_sums(table, 8, [1.0, 3.0]) == 6.5 / 8
    tv1 = (1 + 1e-5) / (1 + 0.3 * 1 + 0.7 * 1.5 + 1e-5)
    assert ls.tversky_from_sums(table) == 1 - tv1
    assert ls.combined_from_sums(table, 2.0, 0.5) == (2 * 4.5 / 8 + 0.5 * (1 - d1), 4.5 / 8, 1 - d1)
    adv = ls.advanced_combined_from_sums(table, 8)
    assert adv[1:] == (2.5 / 8, 1 - tv1, 1 - d1) and adv[0] == 0.4 * adv[1] + 0.4 * adv[2] + 0.2 * adv[3]
    # skip_empty and the fallback: class 1 absent -> nothing valid -> every non-background class again
    empty = table.copy()
    empty[0, 1, [0, 2, 3, 4]] = 0
    e1 = 1e-5 / (2.5 + 1e-5)
    assert ls.dice_from_sums(empty) == 1 - e1 and ls.dice_from_sums(empty, skip_empty=False) == 1 - e1
    # two frames are one batch: the absent class of the second frame is skipped, not averaged
    both = np.concatenate([table, empty])
    assert ls.dice_from_sums(both) == 1 - d1 and ls.dice_from_sums(both, skip_empty=False) == 1 - (d1 + e1) / 2
    with pytest.raises(ValueError):
        ls.cross_entropy_from_sums(table, [1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        ls.dice_from_sums(table[0])


# ---- the header's entries (names, types, build inputs and guard coverage: tests/test_bindings_host.py) ----------------------------------
def test_layout_query():
    import ctypes
    lib = _lib.load()
    span = ctypes.c_int(-1)
    assert lib.unetpp_loss_layout(ctypes.byref(span)) == 0 and span.value > 0 and span.value % 4 == 0
    assert lib.unetpp_loss_layout(None) == -2


def test_header_is_c99(tmp_path):
    cc_ = shutil.which("cc") or shutil.which("gcc")
    assert cc_, "no C compiler"
    src = tmp_path / "use.c"
    src.write_text('#include "unetpp_loss.h"\nint main(void) { uint64_t t[UNETPP_LOSS_COLUMNS] = {0}; (void)t; return UNETPP_LOSS_MAX_CLASSES - 8; }\n')
    subprocess.run([cc_, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True, capture_output=True, text=True)


def test_null_engine_is_refused():
    assert _lib.load().unetpp_loss_sums_f32(None, None, None, 1, 3, 8, 8, 2, None, None, None) == -1


def test_guard_rows_run_at_3_and_7_classes():
    import test_gpu_guarded_loss as tgl
    assert {c for r in tgl.ROWS_LOSS for c in r.classes} >= {3, 7}


# ---- argument checks that need no device --------------------------------------------------------------------------------------------
class _NoDevice:
    """Stands in for the model: the checks under test run before anything reaches the device."""

    def _input(self, t, what="gray", shape="[B,H,W]", dtype="uint8"):
        raise RuntimeError(f"{what} must be a {dtype} CUDA tensor {shape}")


def test_argument_checks():
    import torch
    m = _NoDevice()
    good_l, good_t = np.zeros((2, 3, 8, 8), np.float32), np.zeros((2, 8, 8), np.uint8)
    assert ls.check_args(good_l, good_t, 2) == (2, 3, 8, 8, 2)
    bad = [(np.zeros((2, 3, 8, 8), np.float64), good_t, 2, "float32"), (good_l, np.zeros((2, 8, 8), np.int64), 2, "uint8"),
           (good_l[0], good_t, 2, r"\[B,C,H,W\]"), (good_l, good_t[0], 2, r"\[B,H,W\]"), (good_l, np.zeros((2, 8, 9), np.uint8), 2, "must be equal"),
           (np.zeros((2, 1, 8, 8), np.float32), good_t, 2, "2..8"), (np.zeros((2, 9, 8, 8), np.float32), good_t, 2, "2..8"),
           (good_l, good_t, 5, "gamma"), (good_l, good_t, -1, "gamma"), (good_l, good_t, 2.5, "gamma"), (good_l, good_t, True, "gamma")]
    for lg, tg, gamma, msg in bad:
        with pytest.raises(ValueError, match=msg):
            ls.loss_sums_np(lg, tg, gamma)
        with pytest.raises(ValueError, match=msg):
            ls.loss_sums(m, torch.from_numpy(lg), torch.from_numpy(tg), gamma)
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (1, 2, 2049, 2048), (0, 0, 0, 0))
    with pytest.raises(ValueError, match=r"2\^22"):
        ls.check_args(big, np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), (1, 2049, 2048), (0, 0, 0)))
    # past the shared checks the device form asks the model for its tensors
    with pytest.raises(RuntimeError, match="float32 CUDA tensor"):
        ls.loss_sums(m, torch.from_numpy(good_l), torch.from_numpy(good_t))
    with pytest.raises(RuntimeError, match="float32 CUDA tensor"):
        ls.combined_loss(m, torch.from_numpy(good_l), torch.from_numpy(good_t))
    with pytest.raises(ValueError, match="criterion"):
        ls.evaluate_losses(m, [], criterion="hinge")
    for kind in ("x",):
        with pytest.raises(ValueError):
            ls.make_logits(1, 3, 8, 8, 0, kind)
        with pytest.raises(ValueError):
            ls.make_target(1, 3, 8, 8, 0, kind)
