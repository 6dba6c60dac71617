"""CPU checks of the probability-map rules (unet_amd/probmap.py) against the fixtures made from the reference's own
apply_hysteresis / apply_morphological_and_filtering / scan_thresholds (tests/golden/probmap_scenes.npz,
scripts/make_golden_probmap.py).  Masks, thresholds and every float of the scan's `results`: equality, no tolerance.  The
one condition is on the inputs: no fixture component's mean probability lies within probmap.MEAN_MARGIN of 0.85."""
import hashlib
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import _lib
from unet_amd import evaluation as ev
from unet_amd import probmap as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = load_golden("probmap_scenes")
CASES = [dict(tag=t, H=int(h), W=int(w), seed=int(s), missed=bool(int(m)), sha_p=sp, sha_t=st) for t, h, w, s, m, sp, st in G["cases"]]
TAGS = [c["tag"] for c in CASES]
SETS = [dict(name=n, thr_range=(float(a), float(b), float(c)), tags=tags.split(",")) for n, a, b, c, tags in G["sets"]]
RESULT_KEYS = ("thr", "miou", "precision", "recall", "f1")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def scene(c):
    return pm.make_prob_scene(c["H"], c["W"], c["seed"], c["missed"])


def stored(tag, what, shape):
    return np.unpackbits(G[f"{tag}_{what}"])[:shape[0] * shape[1]].reshape(shape)


def scene_set(s):
    pairs = [scene(CASES[TAGS.index(t)]) for t in s["tags"]]
    return [p for p, _ in pairs], [t for _, t in pairs]


def results_table(results):
    return np.array([[float(r[k]) for k in RESULT_KEYS] for r in results], np.float64)


# ---- 1. the fixtures ------------------------------------------------------------------------------------------------------
def test_scene_generator_reproduces_the_stored_inputs():
    for c in CASES:
        prob, target = scene(c)
        assert prob.dtype == np.float32 and target.dtype == np.uint8 and prob.shape == target.shape == (c["H"], c["W"])
        assert (sha(prob), sha(target)) == (c["sha_p"], c["sha_t"]), c["tag"]
        assert set(np.unique(target)) <= {0, 1} and 0.0 <= prob.min() and prob.max() < 1.0
        for v in (0.9, 0.7):                                  # exact threshold values and their neighbours are in the map
            assert (prob == np.float32(v)).any() or (prob == np.nextafter(np.float32(v), np.float32(0))).any(), (c["tag"], v)


def test_fixture_covers_what_it_should():
    """The generator's own assertions, again: the margin condition for every component; area-only, mean-only and kept
    components; hysteresis growth; a scan whose strategies differ; recall >= 0.9 reached by some thresholds, and by none."""
    totals = np.zeros(5, np.int64)
    for c in CASES:
        prob, _ = scene(c)
        facts = pm.scene_facts(prob, stored(c["tag"], "hyst", prob.shape))
        assert facts[0] >= pm.MEAN_MARGIN, (c["tag"], facts)
        totals += np.array(facts[1:])
    assert (totals > 0).all(), totals
    differ, reach = 0, []
    for s in SETS:
        rec = G[s["name"] + "_results"][:, 3]
        differ += len(set(G[s["name"] + "_thr"].tolist())) > 1
        reach.append((bool((rec >= 0.90).any()), bool((rec < 0.90).any())))
        assert len(rec) == len(pm.scan_values(s["thr_range"])) in (25, 49)
    assert differ >= 1 and (True, True) in reach and (False, True) in reach
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "probmap_scenes.npz")) < 64 * 1024


# ---- 2. the NumPy forms against the reference's results -------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_hysteresis_and_mean_filter_equal_the_reference(tag):
    prob, _ = scene(CASES[TAGS.index(tag)])
    want_h, want_f = stored(tag, "hyst", prob.shape), stored(tag, "final", prob.shape)
    hyst = pm.hysteresis_np(prob[None])
    assert hyst.dtype == np.uint8 and np.array_equal(hyst[0], want_h)
    assert np.array_equal(pm.filter_mean_prob_np(want_h[None], prob[None])[0], want_f)
    both = pm.postprocess_probmap_np(np.stack([1 - prob, prob], -1)[None], channel=1, out_value=255)     # [B,H,W,C] in place
    assert np.array_equal(both[0][0], want_h * 255) and np.array_equal(both[1][0], want_f * 255)


@pytest.mark.parametrize("name", [s["name"] for s in SETS])
def test_scan_equals_the_reference(name):
    s = next(x for x in SETS if x["name"] == name)
    probs, targets = scene_set(s)
    thr_miou, thr_f1, thr_prec90, results = pm.scan_thresholds_np(probs, targets, s["thr_range"])
    assert [float(thr_miou), float(thr_f1), float(thr_prec90)] == G[name + "_thr"].tolist()
    assert np.array_equal(results_table(results), G[name + "_results"])          # every float, ==
    assert all(type(r["thr"]) is np.float64 for r in results)
    # the same thresholds handed over as a list; a float32 array is used as it is
    again = pm.scan_thresholds_np(probs, targets, thresholds=pm.scan_values(s["thr_range"]))
    assert again[:3] == (thr_miou, thr_f1, thr_prec90) and again[3] == results
    t32 = pm.check_thresholds(pm.scan_values(s["thr_range"]))
    assert np.array_equal(results_table(pm.scan_thresholds_np(probs, targets, thresholds=t32)[3])[:, 1:], G[name + "_results"][:, 1:])


# ---- 3. thresholds ----------------------------------------------------------------------------------------------------------
def test_f32_nearest_and_f32_ceil():
    for v in (0.9, 0.7, 0.85, 0.5, 0.25, 1.0, 0.0, 0.59, 0.98, 1e-30, 3.0):
        n, c = pm.f32_nearest(v), pm.f32_ceil(v)
        assert type(n) is np.float32 and type(c) is np.float32 and n == np.float32(v)
        assert float(c) >= v and float(np.nextafter(c, np.float32(-np.inf))) < v     # the smallest float32 not below v
    assert float(pm.f32_nearest(0.9)) < 0.9 < float(pm.f32_ceil(0.9)) and pm.f32_ceil(0.9) == np.nextafter(np.float32(0.9), np.float32(1))
    assert float(pm.f32_nearest(0.7)) < 0.7 and pm.f32_ceil(0.7) == np.nextafter(np.float32(0.7), np.float32(1))
    for exact in (0.5, 0.625, 0.75, 1.0, float(np.float32(0.9))):
        assert float(pm.f32_ceil(exact)) == exact == float(pm.f32_nearest(exact))
        up = float(np.nextafter(np.float32(exact), np.float32(2)))
        down = float(np.nextafter(np.float32(exact), np.float32(0)))
        assert float(pm.f32_ceil((exact + up) / 2)) == up and float(pm.f32_ceil((exact + down) / 2)) == exact
    # what the conversions stand for: NumPy's own comparisons
    p = np.array([np.float32(0.9), np.nextafter(np.float32(0.9), np.float32(1)), np.nextafter(np.float32(0.9), np.float32(0))])
    assert np.array_equal(p >= 0.9, p >= pm.f32_nearest(0.9)) and (p >= 0.9).tolist() == [True, True, False]
    assert np.array_equal(p >= np.float64(0.9), p >= pm.f32_ceil(0.9)) and (p >= np.float64(0.9)).tolist() == [False, True, False]
    for bad in (float("nan"), np.float32("nan")):
        with pytest.raises(ValueError):
            pm.f32_ceil(bad)
        with pytest.raises(ValueError):
            pm.f32_nearest(bad)


def test_thr_q_and_exact_ties():
    assert pm.thr_q_of(0.625) == 5 << 29 and pm.thr_q_of(1.0) == 1 << 32 and pm.thr_q_of(0.0) == 0
    assert pm.thr_q_of(0.85) == int(Fraction(float(np.float32(0.85))) * 2 ** 32) and pm.thr_q_of(0.85) * 2 ** -32 == float(np.float32(0.85))
    assert pm.thr_q_of(1e-12) == 1                             # the ceiling, below 2^-32
    stats = np.zeros((4, 5), np.int32)
    stats[1:, 4] = (8, 8, 3)
    q = pm.q32_np(np.float32([0.5, 0.75, 1.0, 0.0, -1.0, 2.0, np.nan, 1e-45, 2.0 ** -32, 2.0 ** -33, -0.0]))
    assert q.tolist() == [1 << 31, 3 << 30, 1 << 32, 0, 0, 1 << 32, 0, 0, 1, 0, 0]
    tie = 4 * (1 << 31) + 4 * (3 << 30)                        # four 0.5 and four 0.75: mean 0.625 exactly
    sums = np.array([0, tie, tie - 1, 3 << 32], np.uint64)
    assert pm.keep_mean_prob(stats, sums, 4, 0.625).tolist() == [False, True, False, False]      # the tie stays; the third is too small
    assert pm.keep_mean_prob(stats, sums, 3, 0.625).tolist() == [False, True, False, True]
    assert pm.means_from_sums(sums, stats)[1:].tolist() == [0.625, (tie - 1) / 2 ** 32 / 8, 1.0]
    # through the whole NumPy form (kernel_size 1: no morphology): a 4 x 4 block, half 0.5 and half 0.75, then one pixel
    # lowered by an ulp
    mask = np.zeros((1, 8, 8), np.uint8)
    mask[0, 2:6, 2:6] = 1
    prob = np.zeros((1, 8, 8), np.float32)
    prob[0, 2:6, 2:4], prob[0, 2:6, 4:6] = 0.5, 0.75
    assert np.array_equal(pm.filter_mean_prob_np(mask, prob, 16, 0.625, kernel_size=1), mask)
    prob[0, 3, 3] = np.nextafter(np.float32(0.5), np.float32(0))
    assert not pm.filter_mean_prob_np(mask, prob, 16, 0.625, kernel_size=1).any()


# ---- 4. the histogram ---------------------------------------------------------------------------------------------------------
def test_confusion_from_hist_equals_confusion_np_per_threshold():
    c = CASES[0]
    prob, target = scene(c)
    prob = np.stack([prob, prob[::-1]])
    target = np.stack([target, target])
    prob[0, 0, :4] = (np.nan, 2.0, -1.0, -0.0)
    thr = pm.check_thresholds(pm.scan_values())
    total = np.zeros((2 * (len(thr) + 1) + 1,), np.int64)
    hist = pm.threshold_hist_np(prob, target, thr, total=total)
    assert hist.dtype == np.int64 and hist.shape == (2, 2, len(thr) + 1) and hist.sum() == prob.size
    assert np.array_equal(total[:-1].reshape(2, -1), hist.sum(0)) and total[-1] == 0
    cm = pm.confusion_from_hist(hist)
    assert cm.shape == (2, len(thr), 2, 2)
    for j, t in enumerate(thr):
        want, _ = ev.confusion_np((prob >= t).astype(np.uint8), target, 2)
        assert np.array_equal(cm[:, j], want), j
    # target_class, ignore_value, and the float64 comparison of the reference
    t3 = target * np.uint8(3)
    t3[:, :2] = 255
    h2, outside = pm.threshold_hist_np(prob, t3, [0.6, 0.9], target_class=3, ignore_value=255, return_outside=True)
    assert outside.tolist() == [2 * c["W"]] * 2 and h2.sum() + outside.sum() == prob.size
    keep = t3 != 255
    for b in range(2):
        for g in (0, 1):
            sel = keep[b] & ((t3[b] == 3) == bool(g))
            assert h2[b, g, 2] == (sel & (prob[b] >= np.float64(0.9))).sum() and h2[b, g, 0] == (sel & ~(prob[b] >= np.float64(0.6))).sum()


def test_value_errors():
    prob = np.zeros((1, 4, 5), np.float32)
    mask = np.zeros((1, 4, 5), np.uint8)
    with pytest.raises(ValueError, match="thr_low"):
        pm.hysteresis_np(prob, 0.7, 0.9)
    with pytest.raises(ValueError, match="iterations"):
        pm.hysteresis_np(prob, iterations=0)
    with pytest.raises(ValueError, match="t_low"):
        pm.levels_np(prob, 0.9, 0.7)
    with pytest.raises(ValueError, match="float32"):
        pm.levels_np(prob.astype(np.float64), 0.5)
    with pytest.raises(ValueError, match="channel"):
        pm.levels_np(np.zeros((1, 4, 5, 2), np.float32), 0.5)
    with pytest.raises(ValueError, match="channel"):
        pm.levels_np(np.zeros((1, 4, 5, 2), np.float32), 0.5, channel=2)
    with pytest.raises(ValueError, match="channel"):
        pm.levels_np(prob, 0.5, channel=1)
    for bad in ([], [0.5, 0.5], [0.6, 0.5], [0.5, float("nan")], [0.9, 0.9 + 1e-12], np.linspace(0, 1, 257)):
        with pytest.raises(ValueError, match="thresholds"):
            pm.threshold_hist_np(prob, mask, bad)
    with pytest.raises(ValueError, match="target"):
        pm.threshold_hist_np(prob, mask[:, :3], [0.5])
    with pytest.raises(ValueError, match="target_class"):
        pm.threshold_hist_np(prob, mask, [0.5], target_class=256)
    with pytest.raises(ValueError, match="ignore_value"):
        pm.threshold_hist_np(prob, mask, [0.5], ignore_value=-1)
    with pytest.raises(ValueError, match="total"):
        pm.threshold_hist_np(prob, mask, [0.5], total=np.zeros(4, np.int64))
    with pytest.raises(ValueError, match="labels"):
        pm.prob_sums_np(mask, prob, 4)
    with pytest.raises(ValueError, match="mask"):
        pm.filter_mean_prob_np(mask.astype(np.int32), prob)
    with pytest.raises(ValueError, match="integer table"):
        pm.confusion_from_hist(np.zeros((1, 2, 3)))
    with pytest.raises(ValueError, match="empty"):
        pm.scan_thresholds_np([], [])


# ---- 5. the surface -----------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_header_are_listed():
    names = {"unetpp_probmap_layout", "unetpp_prob_levels_f32", "unetpp_prob_threshold_hist_f32", "unetpp_components_prob_sum_f32",
             "unetpp_components_filter_mean"}
    assert names <= set(_lib.ABI_SYMBOLS) and "probmap.h" in _lib.HEADERS
    header = open(os.path.join(ROOT, "include", "unetpp.h")).read()
    assert names <= set(re.findall(r"\b(unetpp_[a-z0-9_]+)\s*\(", header))
    assert os.path.exists(os.path.join(_lib.CSRC, "probmap.h"))


def test_module_imports_without_torch():
    import subprocess
    import sys
    code = ("import sys; sys.modules['torch'] = None\n"
            "import numpy as np\n"
            "from unet_amd import probmap as pm\n"
            "p, t = pm.make_prob_scene(64, 64, 0)\n"
            "h, f = pm.postprocess_probmap_np(p[None])\n"
            "assert h.any() and pm.threshold_hist_np(p[None], t[None], [0.5]).sum() == p.size\n"
            "assert 'torch' not in [m for m in sys.modules if sys.modules[m] is not None]\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


@pytest.mark.parametrize("cls", ["NestedUNet", "SimpleUNet"])
def test_host_tensors_are_refused_before_the_device_is_touched(cls):
    import torch
    from unet_amd import frame_loop, nested_unet
    model = getattr(nested_unet, cls)(2)
    prob = torch.zeros((1, 16, 16), dtype=torch.float32)
    mask = torch.zeros((1, 16, 16), dtype=torch.uint8)
    want = "prob must be a float32 CUDA tensor [B,H,W] or [B,H,W,C]"
    for call in (lambda: pm.threshold_levels(model, prob, 0.5), lambda: pm.hysteresis(model, prob),
                 lambda: pm.filter_by_mean_prob(model, mask, prob), lambda: pm.postprocess_probmap(model, prob),
                 lambda: pm.threshold_histogram(model, prob, mask, [0.5]), lambda: pm.scan_thresholds(model, prob, mask),
                 lambda: pm.component_prob_sums(model, mask.int(), mask.int()[:, 0, 0], prob)):
        with pytest.raises(RuntimeError) as err:
            call()
        assert str(err.value) == want
    with pytest.raises(ValueError, match="thr_low"):
        pm.hysteresis(model, prob, 0.7, 0.9)
    assert callable(frame_loop.process_frames_optimized)
