"""CPU side of the logit-head tests (tests/test_gpu_head_classes.py is the device side).

The last step of both networks, the 1x1 head that turns x0_4 (SimpleUNet: dec1) into logits, probabilities, the argmax mask and
the cable / tape masks (reference src/models/unetpp.py:85,119, simple_unet.py:92,124, infer_two_stage_burr.py:294-304), exists
four times on the device.  Each loops over 8 class slots, pads slots c >= C with -inf and lets the first
maximal class win.  This file holds, without a GPU:

  * the cases of the device tests (shapes, frames, weight seeds) and the proof, on the oracle alone, that they have teeth:
    over the C rotations of a case every class index is the oracle's answer on at least 5 % of the pixels of one rotation; a
    tied pair is the oracle's maximum on at least 25 % of the pixels; the class rules' inputs leave at most 0.5 % of the pixels
    near a decision boundary;
  * the checking functions the device tests import (check_rotation, check_tie, check_constant), and `head_np`, a plain NumPy
    head with a `defect=` switch: every planted defect fails at least one of those checks, the right head passes them all;
  * the small host facts: blob sizes for every class count, the class rules' winner among the first three classes, the
    rotation property of the committed emulations.

The probabilities roll with the head bit for bit as well, because the heads take the softmax denominator as a symmetric function
of the classes (softmax_denominator, csrc/conv3x3_mfma.h: every term rounded to a multiple of 2^-28, the integers added).  A
float32 sum in class order, which the reference's np.sum is and the heads' was, does not have that property once three or more
terms are non-zero (test_the_reference_softmax_is_not_bitwise_rotation_invariant).
"""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_value_range_host import RULES, boundary_distance, softmax64

sys.path.insert(0, os.path.join(ROOT, "oracle"))

SLOTS = 8                                   # HEAD_FUSED_MAX_CLASSES (csrc/conv3x3_mfma.h)
CLASS_COUNTS = tuple(range(1, SLOTS + 1))
NESTED_SHAPES = ((2, 32, 48), (1, 16, 80))  # W no multiple of the 32-pixel tile; two and one tile rows
SIMPLE_SHAPE = (2, 24, 40)
DS_SHAPE = (2, 32, 48)
DS_CLASS_COUNTS = (1, 2, 4, 5, 6, 8)
RULE_CLASS_COUNTS = (4, 5, 6, 8)
RULE_SHAPE = (2, 32, 48)
FRAME_SEED = 7
WEIGHT_SEEDS = {}                           # (arch, C) -> seed where seed 0 misses a condition of this file; none does
COVERAGE = 0.05                             # every class index is the answer on this share of the pixels of some rotation
TIE_SHARE = 0.25                            # a tied pair is the maximum on this share of the pixels
NEAR_CAP = 0.005                            # tests/test_gpu_value_range.py::test_logit_scale: pixels near a rule's boundary


def weight_seed(arch, C):
    return WEIGHT_SEEDS.get((arch, C), 0)


@functools.lru_cache(maxsize=None)
def case(arch, C, shape):
    """(state dict, uint8 frames, float32 NCHW input) of one device case.  The dict is shared: never written."""
    from unet_amd import synthetic as syn
    B, H, W = shape
    sd = syn.make_state_dict(C, 3, True, weight_seed(arch, C)) if arch == "nested" else syn.make_simple_state_dict(C, 3, weight_seed(arch, C))
    frames = syn.make_frames_u8(B, H, W, "smooth", FRAME_SEED)
    return sd, frames, syn.frames_to_chw_f32(frames)


def oracle_forward(arch, sd, x):
    import unetpp_oracle as oracle
    return oracle.torch_forward(sd, x) if arch == "nested" else oracle.simple_unet_torch_forward(sd, x)


@functools.lru_cache(maxsize=None)
def head_input(arch, C, shape):
    """the node the head reads in the oracle's forward (x0_4, SimpleUNet: dec1), float32 [B,Cx,H,W]"""
    import unetpp_oracle as oracle
    sd, _, x = case(arch, C, shape)
    if arch == "nested":
        return oracle.torch_forward(sd, x, return_intermediates=True)[1]["x0_4"]
    return oracle.simple_unet_torch_forward(sd, x, return_intermediates=True)[1]["dec1"]


def oracle_logits(arch, C, shape, sd):
    """the oracle's logits for a state dict that differs from the case's only in its heads: the same F.conv2d call on the same
    node as the oracle's forward makes, hence its bits (checked in test_the_cases_cover_every_class_index), without the trunk"""
    import torch
    import torch.nn.functional as F
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    with torch.no_grad():
        return F.conv2d(T(head_input(arch, C, shape)), T(sd["final.weight"]), T(sd["final.bias"])).numpy()


def argmax_mask(logits):
    return np.argmax(logits, axis=1).astype(np.uint8)


def shares(mask, C):
    return np.bincount(mask.ravel(), minlength=C)[:C] / mask.size


@functools.lru_cache(maxsize=None)
def tie_pair(arch, C, shape):
    """(a, b): the rows that win most and second most pixels of the oracle's mask (b: the first other row if only one wins)"""
    import unetpp_oracle as oracle
    sd = case(arch, C, shape)[0]
    count = np.bincount(oracle.masks_from_logits(oracle_logits(arch, C, shape, sd))[0].ravel(), minlength=C)[:C].astype(np.int64)
    a = int(np.argmax(count))
    rest = count.copy()
    rest[a] = -1
    return a, int(np.argmax(rest))


def rule_rotations(C, shape=RULE_SHAPE):
    """the rotations of the class-rule cases: 0, and the one that puts the row winning most pixels at class index 3"""
    return (0, (3 - tie_pair("nested", C, shape)[0]) % C)


def constant_bias_cases(C):
    """[(tag, biases)] of the constant-logit cases; the expected mask is np.argmax(biases), the first maximal index.
    'increasing' is negative throughout: a slot c >= C padded with 0 where -inf belongs would win it."""
    out = [("equal", [0.5] * C), ("increasing", [-0.25 * (C - c) for c in range(C)])]
    for c in range(C):
        out.append((f"max_from_{c}", [0.25 * i - 3.0 if i < c else 1.0 for i in range(C)]))
    for c in range(C):
        out.append((f"spike_{c}", [80.0 if i == c else -80.0 for i in range(C)]))
    return out


# ----------------------------------------------------------------------------- the checks (shared with the device tests)
# A result is a dict of NumPy arrays: logits [B,C,H,W] f32, probs [B,C,H,W] f32, mask / cable / tape [B,H,W] u8.
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_outputs(res, C):
    """what holds for every result of every head: the mask is np.argmax of the head's own logits, the class masks follow it"""
    lg, mask = res["logits"], res["mask"]
    assert lg.shape[1] == C and res["probs"].shape == lg.shape
    assert np.array_equal(mask, argmax_mask(lg)), "mask is not np.argmax of the logits"
    assert np.array_equal(res["cable"], (mask == 1).astype(np.uint8)), "cable != (mask == 1)"
    assert np.array_equal(res["tape"], (mask == 2).astype(np.uint8)), "tape != (mask == 2)"
    assert np.isfinite(lg).all() and np.isfinite(res["probs"]).all()
    if C == 1:
        assert not mask.any() and (res["probs"] == np.float32(1.0)).all()
    if C <= 2:
        assert not res["tape"].any()


def check_rotation(results, C):
    """results[j]: the result with rotate_head(sd, j) loaded, j = 0 .. C-1 (or a subset as a dict {j: result}, 0 included)"""
    by_j = dict(enumerate(results)) if not isinstance(results, dict) else results
    base = by_j[0]
    seen = set()
    for j, res in by_j.items():
        check_outputs(res, C)
        assert np.array_equal(bits(res["logits"]), bits(np.roll(base["logits"], j, axis=1))), f"logits of rotation {j} are not rotation 0's, rolled"
        assert np.array_equal(bits(res["probs"]), bits(np.roll(base["probs"], j, axis=1))), f"probabilities of rotation {j} are not rotation 0's, rolled"
        seen |= set(np.unique(res["mask"]).tolist())
    if len(by_j) == C:
        assert seen == set(range(C)), f"classes in the masks over all rotations: {sorted(seen)}"


def rotation_prob_mismatch(results, C):
    """(elements, largest difference) of the probabilities of rotation j that are not bitwise rotation 0's, rolled"""
    by_j = dict(enumerate(results)) if not isinstance(results, dict) else results
    n, worst = 0, 0.0
    for j, res in by_j.items():
        want = np.roll(by_j[0]["probs"], j, axis=1)
        differ = bits(res["probs"]) != bits(want)
        n += int(differ.sum())
        worst = max(worst, float(np.abs(res["probs"].astype(np.float64) - want).max()))
    return n, worst


def check_tie(res, C, lo, hi):
    """classes lo < hi hold bit copies of one row and bias"""
    assert 0 <= lo < hi < C
    check_outputs(res, C)
    assert np.array_equal(bits(res["logits"][:, lo]), bits(res["logits"][:, hi])), "the tied logit planes differ"
    assert not (res["mask"] == hi).any(), "the later class of a tied pair won a pixel"
    share = float((res["mask"] == lo).mean())
    assert share >= TIE_SHARE, f"the earlier class of the tied pair wins {share:.1%} of the pixels"
    assert np.array_equal(bits(res["probs"][:, lo]), bits(res["probs"][:, hi])), "the tied probability planes differ"


def check_constant(res, C, tag, biases):
    """constant_head(sd, biases) is loaded: every logit is its bias, the mask the first maximal index"""
    b = np.asarray(biases, np.float32)
    check_outputs(res, C)
    assert (res["logits"] == b[None, :, None, None]).all(), f"{tag}: a logit is not its bias"
    assert (res["mask"] == int(np.argmax(b))).all(), f"{tag}: the mask is not the first maximal index {int(np.argmax(b))}"
    p64 = softmax64(b[None, :, None, None])
    assert float(np.abs(res["probs"] - p64).max()) <= 1e-6, tag
    if tag == "equal":                       # 1.0 / float(C), correctly rounded (hipcc's default for '/'; NumPy's always)
        assert (res["probs"] == np.float32(1.0) / np.float32(C)).all(), tag
    if tag.startswith("spike"):              # exp(-160) is 0 in float32: exactly 1 and 0, and nothing from the -inf slots
        assert (res["probs"] == (b > 0).astype(np.float32)[None, :, None, None]).all(), tag


# ----------------------------------------------------------------------------- a plain head, right or wrong in one way
DEFECTS = ("ge", "bias_at_8", "pad_zero", "row5_from_4", "ordered_sum")


def head_np(x0_4, w, b, C, defect=None):
    """The head as all four kernels state it, in float32 NumPy: an LDS image [C][Cx] weights then [C] biases, 8 class slots,
    slots c >= C padded with -inf, per class the same sequence of float32 operations, first maximal class, then
    exp(x - max) / sum with the sum of softmax_denominator (csrc/conv3x3_mfma.h): terms rounded to multiples of 2^-28, added
    as integers.
    defect: 'ge' (>= where > belongs in the argmax), 'bias_at_8' (bias read at 8 * Cx + c), 'pad_zero' (slots >= C hold 0),
    'row5_from_4' (class 5 reads class 4's weights), 'ordered_sum' (the denominator as a float32 sum in class order)."""
    assert defect is None or defect in DEFECTS
    x = np.asarray(x0_4, np.float32)
    B, Cx, H, W = x.shape
    lds = np.zeros(SLOTS * Cx + SLOTS, np.float32)
    lds[:C * Cx] = np.asarray(w, np.float32).reshape(-1)
    lds[C * Cx:C * Cx + C] = np.asarray(b, np.float32)
    bias_at = (SLOTS if defect == "bias_at_8" else C) * Cx
    lg = np.full((B, SLOTS, H, W), 0.0 if defect == "pad_zero" else -np.inf, np.float32)
    for c in range(C):
        row = 4 if (defect == "row5_from_4" and c == 5) else c
        s = np.zeros((B, H, W), np.float32)
        for ch in range(Cx):
            s = s + x[:, ch] * lds[row * Cx + ch]
        lg[:, c] = lds[bias_at + c] + s
    best, besti = lg[:, 0].copy(), np.zeros((B, H, W), np.uint8)
    for c in range(1, SLOTS):
        take = lg[:, c] >= best if defect == "ge" else lg[:, c] > best
        best, besti = np.where(take, lg[:, c], best), np.where(take, np.uint8(c), besti)
    with np.errstate(invalid="ignore"):
        pe = [np.exp(lg[:, c] - best).astype(np.float32) if c < C else np.zeros((B, H, W), np.float32) for c in range(SLOTS)]
    if defect == "ordered_sum":
        total = np.zeros((B, H, W), np.float32)
        for c in range(SLOTS):
            total = total + pe[c]
    else:
        q = np.zeros((B, H, W), np.uint32)
        for c in range(SLOTS):
            q = q + np.rint(pe[c] * np.float32(2.0 ** 28)).astype(np.uint32)
        total = q.astype(np.float32) * np.float32(2.0 ** -28)
    probs = np.stack([pe[c] / total for c in range(C)], axis=1)
    return {"logits": np.ascontiguousarray(lg[:, :C]), "probs": probs, "mask": besti,
            "cable": (besti == 1).astype(np.uint8), "tape": (besti == 2).astype(np.uint8)}


def run_checks(head, arch, C, shape):
    """checks b (rotation), d (ties) and e (constant logits) of the device file on head(sd) -> result; returns the failures"""
    from unet_amd import synthetic as syn
    sd = case(arch, C, shape)[0]
    failed = {}

    def attempt(name, fn):
        try:
            fn()
        except AssertionError as err:
            failed.setdefault(name, str(err))
    attempt("b", lambda: check_rotation([head(syn.rotate_head(sd, j)) for j in range(C)], C))
    a, b = tie_pair(arch, C, shape)
    tied = syn.tie_head(sd, a, b)
    for j in range(C):
        pair = sorted(((a + j) % C, (b + j) % C))
        attempt("d", lambda: check_tie(head(syn.rotate_head(tied, j)), C, *pair))
    for tag, biases in constant_bias_cases(C):
        attempt("e", lambda: check_constant(head(syn.constant_head(sd, biases)), C, tag, biases))
    return failed


@pytest.mark.parametrize("arch,shape", [("nested", (1, 16, 80)), ("simple", (1, 16, 24))])
def test_planted_defects_fail_the_checks_and_the_right_head_passes(arch, shape, syn):
    """Mutation check of b, d and e at C = 6 (class 5 exists, slots 6 and 7 are padding, 6 * Cx != 8 * Cx), on the oracle's
    own x0_4 (SimpleUNet: dec1, Cx = 64)."""
    C = 6
    node = head_input(arch, C, shape)
    head = lambda defect: (lambda sd: head_np(node, sd["final.weight"][:, :, 0, 0], sd["final.bias"], C, defect))
    assert run_checks(head(None), arch, C, shape) == {}
    caught = {d: sorted(run_checks(head(d), arch, C, shape)) for d in DEFECTS}
    print(f"{arch}: checks failed per planted defect: {caught}")
    assert all(caught.values()), caught
    assert "d" in caught["ge"] and "e" in caught["bias_at_8"] and "e" in caught["pad_zero"] and "b" in caught["row5_from_4"]
    assert caught["ordered_sum"] == ["b"]


# ----------------------------------------------------------------------------- the constructors
def test_head_constructors(syn):
    for sd in (syn.make_state_dict(5, 3, True, 0), syn.make_state_dict(5, 3, False, 0), syn.make_simple_state_dict(5, 3, 0)):
        heads = [h for h in syn.HEAD_NAMES if h + ".weight" in sd]
        assert heads[0] == "final" and len(heads) in (1, 4)
        before = {k: np.array(v, copy=True) for k, v in sd.items()}
        rot, tied, const = syn.rotate_head(sd, 2), syn.tie_head(sd, 3, 1), syn.constant_head(sd, [1, 2, 3, 4, 5])
        for h in heads:
            w, b = sd[h + ".weight"], sd[h + ".bias"]
            for c in range(5):
                assert np.array_equal(bits(rot[h + ".weight"][c]), bits(w[(c - 2) % 5])) and bits(rot[h + ".bias"])[c] == bits(b)[(c - 2) % 5]
            assert np.array_equal(bits(tied[h + ".weight"][1]), bits(w[3])) and bits(tied[h + ".bias"])[1] == bits(b)[3]
            assert all(np.array_equal(tied[h + ".weight"][c], w[c]) and tied[h + ".bias"][c] == b[c] for c in (0, 2, 3, 4))
            assert not bits(const[h + ".weight"]).any()                       # +0.0 everywhere: no sign bit either
            assert const[h + ".bias"].tolist() == [1, 2, 3, 4, 5] and const[h + ".weight"].shape == w.shape
            assert all(d[h + ".weight"].dtype == np.float32 and d[h + ".bias"].dtype == np.float32 and d[h + ".weight"].flags.c_contiguous
                       for d in (rot, tied, const))
        assert np.array_equal(syn.rotate_head(sd, 5)["final.weight"], sd["final.weight"])
        for d in (rot, tied, const):                                           # nothing but the heads differs; the input is untouched
            assert set(d) == set(sd) and all(d[k] is sd[k] for k in sd if k.split(".")[0] not in syn.HEAD_NAMES)
        assert all(np.array_equal(before[k], sd[k]) for k in sd)
    with pytest.raises(ValueError):
        syn.tie_head(sd, 1, 1)
    with pytest.raises(ValueError):
        syn.tie_head(sd, 0, 5)
    with pytest.raises(ValueError):
        syn.constant_head(sd, [0.0] * 4)


# ----------------------------------------------------------------------------- host facts
def test_blob_sizes_for_every_class_count(syn):
    """packing against the library's own size functions, reached as tests/test_ds_host.py reaches them (no device call)"""
    from unet_amd import _lib, packing
    lib = _lib.load()
    for C in CLASS_COUNTS:
        sd = syn.make_state_dict(C, 3, True, 0)
        assert len(packing.build_blob(sd, C)) == lib.unetpp_weights_blob_bytes_arch(_lib.ARCH_NESTED, C, 3) == lib.unetpp_weights_blob_bytes(C, 3)
        assert len(packing.build_simple_blob(syn.make_simple_state_dict(C, 3, 0), C)) == lib.unetpp_weights_blob_bytes_arch(_lib.ARCH_SIMPLE, C, 3)
        assert len(packing.build_ds_blob(sd, C)) == lib.unetpp_ds_blob_bytes(C)
        for rot in (syn.rotate_head(sd, 1), syn.constant_head(sd, [0.5] * C)):
            assert len(packing.build_blob(rot, C)) == len(packing.build_blob(sd, C))
        pay = packing.build_blob(syn.rotate_head(sd, 1), C)[32:].view(np.float32)      # the head is the blob's tail: rows then biases
        assert np.array_equal(pay[-C:], np.roll(sd["final.bias"], 1)) and np.array_equal(pay[-C * 33:-C], np.roll(sd["final.weight"], 1, axis=0).ravel())


def test_rules_take_their_winner_among_the_first_three_classes(oracle):
    """One pixel whose overall maximum is class 5 while class 1 passes thresholded_argmax: cable.  The device's apply_rule sees
    pe[0..2] only (csrc/conv3x3_mfma.h); tests/test_gpu_head_classes.py leans on the oracle doing the same."""
    p = np.array([0.02, 0.46, 0.02, 0.0, 0.0, 0.50], np.float64)
    logits = np.log(np.maximum(p, 1e-30)).astype(np.float32).reshape(1, 6, 1, 1)
    assert int(np.argmax(logits[0, :, 0, 0])) == 5
    cable, tape, probs = oracle.rule_masks_from_logits(logits, "thresholded_argmax", t_cable=0.45, t_tape=0.50, bg_margin=0.15)
    assert np.allclose(probs[0, 0, 0], p, atol=1e-6)
    assert cable.tolist() == [[[1]]] and tape.tolist() == [[[0]]]
    assert oracle.masks_from_logits(logits)[1].tolist() == [[[0]]]               # while the argmax masks say: not cable


# ----------------------------------------------------------------------------- the device cases have teeth
ALL_CASES = [("nested", C, s) for C in CLASS_COUNTS for s in NESTED_SHAPES] + [("simple", C, SIMPLE_SHAPE) for C in CLASS_COUNTS]


def test_the_cases_cover_every_class_index(syn, oracle):
    """Coverage condition: over the C rotations of a case, every class index is the oracle's argmax on >= 5 % of the pixels of
    at least one rotation."""
    import torch
    torch.set_num_threads(8)
    for arch, C, shape in ALL_CASES:
        sd, _, x = case(arch, C, shape)
        best = np.zeros(C)
        for j in range(C):
            rot = syn.rotate_head(sd, j)
            lg = oracle_logits(arch, C, shape, rot)
            if j in (0, 1) and C in (1, 5, 8):                                   # the head alone has the bits of the whole forward
                assert np.array_equal(bits(lg), bits(oracle_forward(arch, rot, x)))
            best = np.maximum(best, shares(oracle.masks_from_logits(lg)[0], C))
        base = shares(oracle.masks_from_logits(oracle_logits(arch, C, shape, sd))[0], C)
        print(f"{arch} C={C} {shape} seed {weight_seed(arch, C)}: shares at rotation 0 {np.round(base, 3).tolist()}, "
              f"largest share of each index over the rotations {np.round(best, 3).tolist()}")
        assert best.min() >= COVERAGE, (arch, C, shape)


def test_a_tied_pair_is_on_top_often_enough(syn, oracle):
    """Tie condition: after tie_head(sd, a, b) the oracle's two logit planes are equal and the pair is its maximum on >= 25 %
    of the pixels -- under every rotation, the earlier index of the pair then being np.argmax's answer there."""
    for arch, C, shape in ALL_CASES:
        if C < 2:
            continue
        sd = case(arch, C, shape)[0]
        a, b = tie_pair(arch, C, shape)
        tied = syn.tie_head(sd, a, b)
        order = set()
        for j in range(C):
            lg = oracle_logits(arch, C, shape, syn.rotate_head(tied, j))
            ja, jb = (a + j) % C, (b + j) % C
            order.add(ja < jb)
            assert np.array_equal(lg[:, ja], lg[:, jb])
            mask = oracle.masks_from_logits(lg)[0]
            assert not (mask == max(ja, jb)).any()
            share = float((mask == min(ja, jb)).mean())
            assert share >= TIE_SHARE, (arch, C, shape, j, share)
        assert order == {True, False}                                            # the original row first, and the copy first
        print(f"{arch} C={C} {shape}: rows {a} and {b} tied, on top of {share:.1%} of the pixels")


def test_rule_cases_leave_few_pixels_near_a_boundary(syn, oracle):
    """The class rules at C > 3: the oracle's probabilities (float32 against float64 softmax) and the committed exact8
    emulation's (the largest probability error the device test meets) both leave at most 0.5 % of the pixels within twice their
    error of a decision boundary, and one of the two rotations has a class >= 3 on top of most pixels."""
    import exact8_emulation as em8
    for C in RULE_CLASS_COUNTS:
        sd, _, x = case("nested", C, RULE_SHAPE)
        js = rule_rotations(C)
        assert js[1] != 0 or tie_pair("nested", C, RULE_SHAPE)[0] == 3
        for j in js:
            rot = syn.rotate_head(sd, j)
            ref = oracle_logits("nested", C, RULE_SHAPE, rot)
            p64 = softmax64(ref)
            top = shares(argmax_mask(ref), C)
            if j == js[1]:
                assert top[3] > 0.5, (C, j, top)
            p8 = softmax64(em8.exact8_forward(rot, x))
            d8 = float(np.abs(p8 - p64).max())
            for rule, params in RULES:
                _, _, p32 = oracle.rule_masks_from_logits(ref, rule, **params)
                d = float(np.abs(np.transpose(p32, (0, 3, 1, 2)) - p64).max())
                near = float((boundary_distance(p64, rule, params) <= 2 * d).mean())
                near8 = float((boundary_distance(p64, rule, params) <= 2 * d8).mean())
                print(f"C={C} rotation {j} {rule}: {near:.3%} of the pixels within 2 x {d:.1e} of a boundary, {near8:.3%} within 2 x {d8:.1e} (exact8 emulation)")
                assert d < 1e-6 and near <= NEAR_CAP and near8 <= NEAR_CAP, (C, j, rule)


def test_the_reference_softmax_is_not_bitwise_rotation_invariant(syn, oracle):
    """Why the heads do not take the softmax denominator as the reference does: the logits of a rotated head are the rolled
    logits bit for bit, exp(x - max) is too, but np.sum over the classes in class order (infer_video_3class_best.py:50-53,
    oracle.softmax_last_np) is a float32 sum whose rounding depends on the order of three or more terms, so the reference's own
    probabilities of a checkpoint with permuted head rows differ from the permuted probabilities in the last bit.  With one or
    two classes they cannot.  Either sum is within 2 C 2^-24 of the other, far inside the probabilities' bar (1e-6)."""
    for C in CLASS_COUNTS:
        sd = case("nested", C, NESTED_SHAPES[0])[0]
        lg = oracle_logits("nested", C, NESTED_SHAPES[0], sd)
        p = oracle.softmax_np(lg)
        differ, worst = 0, 0.0
        for j in range(C):
            pj = oracle.softmax_np(np.roll(lg, j, axis=1))
            differ += int((bits(pj) != bits(np.roll(p, j, axis=1))).sum())
            worst = max(worst, float(np.abs(pj - np.roll(p, j, axis=1)).max()))
        print(f"C={C}: {differ} of {C * p.size} probabilities differ from the rolled ones, by at most {worst:.1e}")
        assert worst <= 2 * C * 2.0 ** -24                                       # a float32 sum of C terms in two orders, and the division
        assert differ == 0 if C <= 2 else differ > 0, C


@pytest.mark.parametrize("C", [2, 5, 8])
def test_the_emulations_roll_with_the_head(C, syn):
    """oracle/fast_emulation.py and oracle/exact8_emulation.py take any class count; their logits of rotate_head(sd, j) are the
    rolled logits (the fused and the stand-alone head of `fast`, the fp32 head of exact8)."""
    import exact8_emulation as em8
    import fast_emulation as emf
    sd, _, x = case("nested", C, (1, 16, 80))
    for forward in (em8.exact8_forward, emf.fast_forward, lambda s, v: emf.fast_forward(s, v, fused_head=False)):
        base = forward(sd, x)
        assert base.shape == (1, C, 16, 80)
        for j in (1, C - 1):
            assert np.array_equal(forward(syn.rotate_head(sd, j), x), np.roll(base, j, axis=1)), (C, j)
