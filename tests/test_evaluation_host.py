"""CPU checks of the evaluation restatement (unet_amd/evaluation.py) against the fixtures made from the reference's own
compute_metrics / compute_confusion_matrix / iou_per_class (tests/golden/eval_scenes.npz, scripts/make_golden_eval.py).
Everything is an integer or a quotient of two integers: equality everywhere, no tolerance."""
import hashlib

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import evaluation as ev

IGNORE_INDICES = (-1, 0, 2)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def golden():
    return load_golden("eval_scenes")


def cases(g):
    for tag, C, B, H, W, seed, variant, sha_p, sha_t in g["cases"]:
        yield tag, int(C), int(B), int(H), int(W), int(seed), variant, sha_p, sha_t


def pack(result, C):
    """compute_metrics' tuple in the fixture's layout: mIoU, then precision, recall, IoU per class, -1.0 for no entry."""
    miou, precision, recall, iou = result
    return np.array([miou] + [float(d.get(c, -1.0)) for d in (precision, recall, iou) for c in range(C)], np.float64)


# ---- 1. the fixtures ------------------------------------------------------------------------------------------------------
def test_fixture_covers_what_it_should(golden):
    rows = list(cases(golden))
    assert {r[1] for r in rows} == {3, 7}
    assert {r[6] for r in rows} == set(ev.EVAL_VARIANTS)
    assert (3, 2, 24, 40) in {r[1:5] for r in rows}
    for C in (3, 7):
        assert len({r[3:5] for r in rows if r[1] == C and r[6] == "plain"}) >= 3
    assert max(r[3] for r in rows) <= 96 and max(r[4] for r in rows) <= 200


def test_scene_generators_reproduce_the_stored_inputs(golden):
    for tag, C, B, H, W, seed, variant, sha_p, sha_t in cases(golden):
        pred, target = ev.make_eval_batch(B, H, W, seed, C, variant)
        assert pred.dtype == target.dtype == np.uint8 and pred.shape == target.shape == (B, H, W)
        assert (sha(pred), sha(target)) == (sha_p, sha_t), tag


def test_confusion_np_equals_the_references_matrix(golden):
    for tag, C, B, H, W, seed, variant, _, _ in cases(golden):
        pred, target = ev.make_eval_batch(B, H, W, seed, C, variant)
        counts, outside = ev.confusion_np(pred, target, C)
        assert counts.dtype == outside.dtype == np.int64 and counts.shape == (B, C, C) and outside.shape == (B, 2)
        assert np.array_equal(counts.sum(0), golden[tag + "_cm"]), tag
        assert not outside.any()


def test_metrics_from_confusion_equals_every_stored_tuple(golden):
    n = 0
    for tag, C, B, H, W, seed, variant, _, _ in cases(golden):
        pred, target = ev.make_eval_batch(B, H, W, seed, C, variant)
        counts, _ = ev.confusion_np(pred, target, C)
        for k in IGNORE_INDICES:
            got, want = pack(ev.metrics_from_confusion(counts, k), C), golden[f"{tag}_m{k}"]
            assert got.shape == want.shape and bool((got == want).all()), (tag, k, got, want)     # == on the floats
            assert np.array_equal(pack(ev.metrics_from_confusion(golden[tag + "_cm"], k), C), want)
            n += 1
    assert n == 3 * len(golden["cases"])


def test_reference_behaviours(golden):
    # background stays out of the mean; an absent class: IoU / precision 1.0 or 0.0, recall 1.0; ignore_index skips a class
    cm = np.array([[50, 0, 0], [0, 0, 0], [4, 0, 6]])             # class 1 absent everywhere
    miou, precision, recall, iou = ev.metrics_from_confusion(cm)
    assert (iou[1], precision[1], recall[1]) == (1.0, 1.0, 1.0) and iou[2] == 6 / 10.0 and miou == (1.0 + 0.6) / 2
    cm = np.array([[50, 3, 0], [0, 0, 0], [4, 0, 6]])             # class 1 predicted, never in the target
    miou, precision, recall, iou = ev.metrics_from_confusion(cm)
    assert (iou[1], precision[1], recall[1]) == (0.0, 0.0, 1.0) and miou == (0.0 + 0.6) / 2
    cm = np.array([[50, 0, 0], [5, 0, 0], [0, 0, 6]])             # class 1 in the target, never predicted
    _, precision, recall, iou = ev.metrics_from_confusion(cm)
    assert (iou[1], precision[1], recall[1]) == (0.0, 0.0, 0.0)
    miou, precision, _, iou = ev.metrics_from_confusion(cm, ignore_index=1)
    assert sorted(iou) == [0, 2] == sorted(precision) and miou == 1.0
    assert ev.metrics_from_confusion(np.array([[7, 0], [0, 0]]), ignore_index=1)[0] == 0.0      # nothing left in the mean
    types = ev.metrics_from_confusion(cm)
    assert type(types[0]) is float and all(type(v) is float for d in types[1:] for v in d.values())


def iou_direct(pred, target, C):
    out = np.zeros((C,))
    for c in range(C):
        inter = int(((pred == c) & (target == c)).sum())
        union = int(((pred == c) | (target == c)).sum())
        out[c] = inter / union if union > 0 else 1.0
    return out


def test_iou_per_class_matches_the_definition_and_the_fixture(golden):
    assert str(golden["iou_per_class_source"]) == "tools/eval.py"
    for tag, C, B, H, W, seed, variant, _, _ in cases(golden):
        pred, target = ev.make_eval_batch(B, H, W, seed, C, variant)
        counts, _ = ev.confusion_np(pred, target, C)
        got = np.stack([ev.iou_per_class_from_confusion(f) for f in counts])
        assert got.dtype == np.float64
        assert np.array_equal(got, np.stack([iou_direct(pred[b], target[b], C) for b in range(B)])), tag
        assert np.array_equal(got, golden[tag + "_ipc"]), tag
    assert np.array_equal(ev.iou_per_class_from_confusion(np.zeros((3, 3), np.int64)), np.ones(3))


# ---- 2. confusion_np's bookkeeping ----------------------------------------------------------------------------------------
def test_pixels_are_conserved_and_go_to_the_right_counter():
    pred, target = ev.make_eval_batch(3, 17, 23, 11, 3)
    r = np.random.default_rng(5)
    target[r.random(target.shape) < 0.1] = 255                    # ignored
    pred[r.random(pred.shape) < 0.05] = 9                         # invalid in the pred
    target[r.random(target.shape) < 0.05] = 3                     # invalid in the target (3 >= C)
    counts, outside = ev.confusion_np(pred, target, 3, ignore_value=255)
    assert np.array_equal(counts.sum((1, 2)) + outside.sum(1), np.full(3, 17 * 23))
    assert np.array_equal(outside[:, 0], (target == 255).sum((1, 2)))
    assert np.array_equal(outside[:, 1], ((target != 255) & ((target >= 3) | (pred >= 3))).sum((1, 2)))
    assert outside.min() > 0
    for t in range(3):
        for p in range(3):
            assert np.array_equal(counts[:, t, p], ((target == t) & (pred == p)).sum((1, 2)))
    # without an ignore value the 255s are invalid
    _, outside2 = ev.confusion_np(pred, target, 3)
    assert not outside2[:, 0].any() and np.array_equal(outside2[:, 1], outside.sum(1))


def test_an_ignored_target_with_an_invalid_pred_counts_as_ignored_only():
    target = np.array([[[255, 0, 1]]], np.uint8)
    pred = np.array([[[200, 200, 1]]], np.uint8)
    counts, outside = ev.confusion_np(pred, target, 2, ignore_value=255)
    assert outside.tolist() == [[1, 1]] and counts.tolist() == [[[0, 0], [0, 1]]]
    counts, outside = ev.confusion_np(pred, target, 2, ignore_value=0)       # a class can be the ignore value
    assert outside.tolist() == [[1, 1]] and counts.sum() == 1


def test_total_accumulates():
    total = np.zeros((3 * 3 + 2,), np.int64)
    a = ev.confusion_np(*ev.make_eval_batch(2, 9, 11, 1, 3), 3, total=total)
    b = ev.confusion_np(*ev.make_eval_batch(1, 9, 11, 5, 3), 3, total=total)
    assert np.array_equal(total[:9].reshape(3, 3), a[0].sum(0) + b[0].sum(0)) and total.sum() == 3 * 9 * 11


# ---- 3. disagreement_np ----------------------------------------------------------------------------------------------------
def test_disagreement_identical_and_planted():
    a = ev.make_eval_batch(2, 5, 7, 3, 3)[0]
    d = ev.disagreement_np(a, a.copy())
    assert d["n_diff"].tolist() == [0, 0] and d["first"].tolist() == [-1, -1] and set(d) == {"n_diff", "first"}
    b = a.copy()
    b[1, 3, 4] ^= 1
    b[1, 4, 6] ^= 1
    d = ev.disagreement_np(a, b)
    assert d["n_diff"].tolist() == [0, 2] and d["first"].tolist() == [-1, 3 * 7 + 4]


def test_disagreement_margin_nan_and_values_outside_the_logits():
    a = np.array([[[0, 1, 2, 0]]], np.uint8)
    b = np.array([[[1, 1, 0, 2]]], np.uint8)
    lg = np.zeros((1, 3, 1, 4), np.float32)
    lg[0, :, 0, 0] = (0.5, 0.25, 9.0)                              # |0.5 - 0.25|; class 2 is not involved
    lg[0, :, 0, 1] = (0.0, 100.0, -100.0)                          # an equal pixel: never looked at
    lg[0, :, 0, 2] = (1.5, 0.0, -2.0)                              # |-2 - 1.5| = 3.5
    lg[0, :, 0, 3] = (np.nan, 0.0, 1.0)                            # NaN margin
    d = ev.disagreement_np(a, b, lg)
    assert d["n_diff"].tolist() == [3] and d["first"].tolist() == [0]
    assert d["max_margin"].dtype == np.float32 and d["max_margin"].tolist() == [3.5] and d["n_nan"].tolist() == [1]
    b[0, 0, 2] = 7                                                 # a value >= C: counted, left out of the margin
    d = ev.disagreement_np(a, b, lg)
    assert d["n_diff"].tolist() == [3] and d["max_margin"].tolist() == [0.25] and d["n_nan"].tolist() == [1]
    d = ev.disagreement_np(a, a, lg)
    assert d["max_margin"].tolist() == [0.0] and d["n_nan"].tolist() == [0]


# ---- 4. argument errors ----------------------------------------------------------------------------------------------------
def test_argument_errors():
    pred, target = ev.make_eval_batch(1, 4, 5, 0, 3)
    for C in (1, 17, 0, -3):
        with pytest.raises(ValueError, match="num_classes"):
            ev.confusion_np(pred, target, C)
    for ign in (-1, 256):
        with pytest.raises(ValueError, match="ignore_value"):
            ev.confusion_np(pred, target, 3, ignore_value=ign)
    with pytest.raises(ValueError, match="shapes must be equal"):
        ev.confusion_np(pred, target[:, :, :4], 3)
    with pytest.raises(ValueError, match=r"uint8 \[B,H,W\]"):
        ev.confusion_np(pred[0], target[0], 3)
    with pytest.raises(ValueError, match=r"uint8 \[B,H,W\]"):
        ev.confusion_np(pred.astype(np.int32), target, 3)
    for total in (np.zeros((10,), np.int64), np.zeros((12,), np.int64), np.zeros((11,), np.int32), np.zeros((11,), np.uint64),
                  np.zeros((1, 11), np.int64)):
        with pytest.raises(ValueError, match="total must be int64"):
            ev.confusion_np(pred, target, 3, total=total)
    with pytest.raises(ValueError, match="shapes must be equal"):
        ev.disagreement_np(pred, target[:, :3])
    with pytest.raises(ValueError, match="logits"):
        ev.disagreement_np(pred, target, np.zeros((1, 3, 4, 6), np.float32))
    with pytest.raises(ValueError, match="logits"):
        ev.disagreement_np(pred, target, np.zeros((1, 3, 4, 5), np.float64))
    with pytest.raises(ValueError, match="integer table"):
        ev.metrics_from_confusion(np.zeros((3, 3)))
    with pytest.raises(ValueError, match="variant"):
        ev.make_eval_batch(1, 4, 5, 0, 3, "other")


def test_scene_is_piecewise_constant_with_moved_boundaries_and_flips():
    pred, target = ev.make_eval_scene(64, 96, 3, 3)
    same = (target[:, :-1] == target[:, 1:]).mean()
    assert same > 0.95 and 0.03 < (pred != target).mean() < 0.25 and set(np.unique(target)) == {0, 1, 2}
    clean = ev.make_eval_scene(64, 96, 3, 3, flip=0.0)[0]
    assert 0 < (clean != target).mean() < (pred != target).mean()         # the boundary band alone
    ign = ev.make_eval_scene(64, 96, 3, 3, ignore=0.1)[1]
    assert 0.05 < (ign == 255).mean() < 0.15
    again = ev.make_eval_scene(64, 96, 3, 3)
    assert np.array_equal(again[0], pred) and np.array_equal(again[1], target)


def test_module_imports_without_torch():
    import subprocess
    import sys
    code = ("import sys; sys.modules['torch'] = None\n"
            "from unet_amd import evaluation as ev\n"
            "c, o = ev.confusion_np(*ev.make_eval_batch(1, 4, 5, 0, 3), 3)\n"
            "assert c.sum() == 20 and 'torch' not in [m for m in sys.modules if sys.modules[m] is not None]\n")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)


@pytest.mark.parametrize("cls", ["NestedUNet", "SimpleUNet"])
def test_host_tensors_are_refused_before_the_device_is_touched(cls):
    import torch
    from unet_amd import nested_unet
    model = getattr(nested_unet, cls)(3)
    mask = torch.zeros((1, 16, 16), dtype=torch.uint8)
    with pytest.raises(RuntimeError) as err:
        ev.confusion(model, mask, mask)
    assert str(err.value) == "pred must be a uint8 CUDA tensor [B,H,W]"
    with pytest.raises(RuntimeError) as err:
        ev.mask_disagreement(model, mask, mask)
    assert str(err.value) == "a must be a uint8 CUDA tensor [B,H,W]"
    with pytest.raises(ValueError, match="at least one batch"):
        ev.evaluate_batches(model, [])
