"""The logit head at every class count, class index and exact tie (tests/test_head_classes_host.py is the CPU
side: the cases, the proof that they have teeth, and the checking functions, which there also run against planted defects).

The 1x1 head (reference src/models/unetpp.py:85,119, simple_unet.py:92,124; softmax / argmax / class masks of
infer_two_stage_burr.py:294-304) is written four times: fused into conv0_4.conv2's epilogue in the wave-specialised kernel
(`exact`, `exact8`) and in the lock-step kernel (`fast`), stand-alone as head_generic_kernel (SimpleUNet, debug_keep_intermediates,
the low-resolution ds logits), and behind ds_upsample_kernel (deep-supervision and pruned outputs).  For C = 1 .. 8 and all three
precisions: which head ran (a), every class index as the answer through rotate_head (b), the same through the stand-alone head
(c), exact ties through tie_head (d), constant logits through constant_head (e), the ds outputs (f) and the class rules (g).

Measured on an MI355X, fused against stand-alone head on the same weights (c), max |dlogit| over both shapes and rotations 0
and 1: `exact` 1.43e-6 (C = 3) and 1.76e-6 (C = 7), 1.43e-6 ... 1.76e-6 over C = 1 .. 8, under the 2e-6 it is held to; `exact8`
2.86e-5 (C = 3) and 4.57e-5 (C = 7): the stand-alone head reads x0_4 back from its stored (hi, lo8) form; `fast` 5.28e-4 and
7.71e-4: it reads the fp16 plane where the fused head has fp32 registers.  The bar of `exact8` and `fast` is twice the larger
of their two figures (HEAD_UNFUSED_MEASURED): 9.15e-5 and 1.54e-3.

The probabilities roll bitwise too (b): the heads add the softmax terms as integers (softmax_denominator, csrc/conv3x3_mfma.h).
With the denominator as a float32 sum in class order, as the reference's np.sum takes it and the heads did before, 3,442 of
27,648 probabilities differed from the rolled ones at C = 3 and 65,746 of 196,608 at C = 8 (`exact`, 2 x 32 x 48; none at
C = 1, 2), by at most 2.4e-7.
Run on the GPU box:  python -m pytest tests -m gpu"""
import numpy as np
import pytest

from test_gpu_deep_supervision import DS
from test_gpu_deep_supervision import EXACT_TOL as DS_EXACT_TOL
from test_gpu_deep_supervision import LOGIT_TOL as DS_LOGIT_TOL
from test_gpu_deep_supervision import oracle_ds, unexplained_flips
from test_gpu_exact8 import LOGIT_TOL, gate
from test_gpu_parity import EXACT_TOL, FAST_TOL, HEAD_UNFUSED_TOL, SIMPLE_EXACT_TOL, SIMPLE_FAST_TOL, report
from test_head_classes_host import (CLASS_COUNTS, DS_CLASS_COUNTS, DS_SHAPE, NEAR_CAP, NESTED_SHAPES, RULE_CLASS_COUNTS, RULE_SHAPE,
                                    SIMPLE_SHAPE, bits, case, check_constant, check_outputs, check_rotation, check_tie,
                                    constant_bias_cases, oracle_logits, rotation_prob_mismatch, rule_rotations, tie_pair)
from test_value_range_host import RULES, boundary_distance, softmax64

pytestmark = pytest.mark.gpu

PRECISIONS = ("exact", "exact8", "fast")
# (c) max |fused - stand-alone| logits measured on the device at the shapes of this file, per precision and class count
HEAD_UNFUSED_MEASURED = {"exact8": {3: 2.861e-5, 7: 4.573e-5}, "fast": {3: 5.285e-4, 7: 7.713e-4}}
HEAD_UNFUSED_BAR = {"exact": HEAD_UNFUSED_TOL, "exact8": 2 * max(HEAD_UNFUSED_MEASURED["exact8"].values()),
                    "fast": 2 * max(HEAD_UNFUSED_MEASURED["fast"].values())}
FUSED_LABEL = {"exact": "|conv3x3_ws_kernel<", "exact8": "|conv3x3_ws_kernel<", "fast": "|conv3x3_bias_relu_kernel<"}
GENERIC_P = {"exact": 2, "exact8": 3, "fast": 1}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def engines(torch_cuda):
    """one engine per (architecture, class count, precision), sized for every shape of this file; each case loads its own
    state dict into it"""
    from unet_amd.nested_unet import NestedUNet, SimpleUNet
    cache = {}

    def get(arch, C, precision):
        key = (arch, C, precision)
        if key not in cache:
            if arch == "nested":
                m = NestedUNet(C, deep_supervision=True, precision=precision, max_batch=2, max_hw=(32, 80))
            else:
                m = SimpleUNet(C, 3, precision=precision, max_batch=2, max_hw=SIMPLE_SHAPE[1:])
            cache[key] = m.to("cuda:0").eval()
        return cache[key]
    yield get
    cache.clear()


@pytest.fixture(scope="module")
def inputs(torch_cuda):
    """device copy of a case's float32 input, per (architecture, shape)"""
    cache = {}

    def get(arch, shape):
        if (arch, shape) not in cache:
            cache[(arch, shape)] = torch_cuda.from_numpy(case(arch, 1, shape)[2]).cuda()      # the frames do not depend on C
        return cache[(arch, shape)]
    yield get
    cache.clear()


def run(torch, model, xt, keep=False, output=0):
    """one result of the weights the model holds: logits, probabilities, mask, cable and tape as NumPy arrays"""
    model.debug_keep_intermediates(keep)
    mask, cable, tape, logits = model.segment(xt, return_logits=True, return_class_masks=True, output=output)
    probs = model.predict_proba(xt, output=output)
    torch.cuda.synchronize()
    return {"logits": logits.cpu().numpy(), "probs": probs.cpu().numpy(), "mask": mask.cpu().numpy(),
            "cable": cable.cpu().numpy(), "tape": tape.cpu().numpy()}


def launches(model, fn):
    model.profile(True)
    fn()
    names = [r[0] for r in model.profile_read()]
    model.profile(False)
    return names


def shapes_of(arch):
    return NESTED_SHAPES if arch == "nested" else (SIMPLE_SHAPE,)


def against_oracle(tag, arch, precision, res, ref, oracle):
    """rotation 0 against the oracle, at the bars this mode already has in test_gpu_parity.py / test_gpu_exact8.py; then the
    probabilities against a float64 softmax of the oracle's logits at test_logit_scale's bars"""
    ref_mask = oracle.masks_from_logits(ref)[0]
    if precision == "exact8":
        err, _ = gate(tag, res["logits"], res["mask"], ref, ref_mask, oracle, tol=LOGIT_TOL)
    else:
        err, flips, unexplained = report(res["logits"], res["mask"], ref, ref_mask, oracle)
        tol = {("nested", "exact"): EXACT_TOL, ("nested", "fast"): FAST_TOL, ("simple", "exact"): SIMPLE_EXACT_TOL, ("simple", "fast"): SIMPLE_FAST_TOL}
        print(f"{tag}: max|dlogit|={err:.3e} flips={flips} unexplained={unexplained}")
        assert err < tol[(arch, precision)] and unexplained == 0, tag
    perr = float(np.abs(res["probs"] - softmax64(ref)).max())
    rowsum = float(np.abs(res["probs"].astype(np.float64).sum(axis=1) - 1.0).max())
    print(f"{tag}: max|dprob|={perr:.2e} |row sum - 1|={rowsum:.1e}")
    assert perr <= 0.5 * err + 1e-6, tag
    assert rowsum <= 8 * 2.0 ** -23, tag


# ----------------------------------------------------------------------------- a. which head ran
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C", CLASS_COUNTS)
def test_which_head_ran(C, precision, torch_cuda, engines, inputs):
    torch = torch_cuda
    m = engines("nested", C, precision)
    m.load_state_dict(case("nested", C, NESTED_SHAPES[0])[0], strict=True)
    xt = inputs("nested", NESTED_SHAPES[0])
    m.debug_keep_intermediates(False)
    m(xt)
    torch.cuda.synchronize()
    heads = lambda names: [n for n in names if "final" in n or "|head_generic_kernel" in n or "|ds_upsample_kernel" in n]
    fused = heads(launches(m, lambda: m.segment(xt)))
    assert len(fused) == 1 and fused[0].startswith("conv0_4.conv2+final+argmax" + FUSED_LABEL[precision]), fused
    m.debug_keep_intermediates(True)
    alone = heads(launches(m, lambda: m.segment(xt)))
    m.debug_keep_intermediates(False)
    assert alone == [f"final+argmax|head_generic_kernel<{GENERIC_P[precision]}>"], alone
    for k, head, _ in DS:
        names = heads(launches(m, lambda: m.segment(xt, output=k)))
        assert names == [f"{head}|head_generic_kernel<{GENERIC_P[precision]}>", f"{head}+up|ds_upsample_kernel"], (k, names)
    s = engines("simple", C, precision)
    s.load_state_dict(case("simple", C, SIMPLE_SHAPE)[0], strict=True)
    xs = inputs("simple", SIMPLE_SHAPE)
    s(xs)
    torch.cuda.synchronize()
    assert heads(launches(s, lambda: s.segment(xs))) == [f"final+argmax|head_generic_kernel<{GENERIC_P[precision]}>"]


# ----------------------------------------------------------------------------- b. rotation
ROTATIONS = {}


def rotation_results(arch, C, precision, torch, engines, inputs, syn):
    """{shape: [result of rotate_head(sd, j) for j in 0 .. C-1]} through the head an ordinary call takes; computed once"""
    key = (arch, C, precision)
    if key not in ROTATIONS:
        m = engines(arch, C, precision)
        out = {shape: [] for shape in shapes_of(arch)}
        for j in range(C):
            m.load_state_dict(syn.rotate_head(case(arch, C, shapes_of(arch)[0])[0], j), strict=True)
            for shape in out:
                out[shape].append(run(torch, m, inputs(arch, shape)))
        assert m.status() == 0
        ROTATIONS[key] = out
    return ROTATIONS[key]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C", CLASS_COUNTS)
@pytest.mark.parametrize("arch", ["nested", "simple"])
def test_rotation(arch, C, precision, torch_cuda, engines, inputs, syn, oracle):
    """Every class index is the answer somewhere: logits of rotation j are bitwise rotation 0's, rolled; the mask is np.argmax of
    the device's own logits; every class appears over the rotations; rotation 0 is the oracle's within the mode's bars."""
    for shape, results in rotation_results(arch, C, precision, torch_cuda, engines, inputs, syn).items():
        check_rotation(results, C)
        ref = oracle_logits(arch, C, shape, case(arch, C, shape)[0])
        against_oracle(f"{arch} C={C} {shape} {precision}", arch, precision, results[0], ref, oracle)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C", CLASS_COUNTS)
@pytest.mark.parametrize("arch", ["nested", "simple"])
def test_rotation_probabilities(arch, C, precision, torch_cuda, engines, inputs, syn):
    """The probabilities of rotation j are bitwise rotation 0's, rolled: the softmax denominator does not depend on which class
    holds which logit.  The figures are printed first; the first bound is what two float32 sums of C terms and the division
    could differ by (2 C 2^-24)."""
    for shape, results in rotation_results(arch, C, precision, torch_cuda, engines, inputs, syn).items():
        n, worst = rotation_prob_mismatch(results, C)
        print(f"{arch} C={C} {shape} {precision}: {n} of {C * results[0]['probs'].size} probabilities differ from the rolled ones, by at most {worst:.1e}")
        assert worst <= 2 * C * 2.0 ** -24
        assert n == 0


# ----------------------------------------------------------------------------- c. the same through the stand-alone head
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C", CLASS_COUNTS)
def test_standalone_head_rotation_and_fused_agreement(C, precision, torch_cuda, engines, inputs, syn, oracle):
    """debug_keep_intermediates: x0_4 is stored and head_generic_kernel reads it back.  Rotations 0 and 1 roll bitwise; fused and
    stand-alone logits agree within 2e-6 in `exact` (test_exact_matches_golden_small), within HEAD_UNFUSED_BAR otherwise.
    (SimpleUNet only has the stand-alone head: test_rotation[simple-...] is this test for Cx = 64.)"""
    torch = torch_cuda
    m = engines("nested", C, precision)
    fused = rotation_results("nested", C, precision, torch, engines, inputs, syn)
    alone = {shape: {} for shape in NESTED_SHAPES}
    for j in (0, 1) if C > 1 else (0,):
        m.load_state_dict(syn.rotate_head(case("nested", C, NESTED_SHAPES[0])[0], j), strict=True)
        for shape in NESTED_SHAPES:
            alone[shape][j] = run(torch, m, inputs("nested", shape), keep=True)
    m.debug_keep_intermediates(False)
    worst = 0.0
    for shape in NESTED_SHAPES:
        check_rotation(alone[shape], C)
        for j in alone[shape]:
            worst = max(worst, float(np.abs(alone[shape][j]["logits"] - fused[shape][j]["logits"]).max()))
        against_oracle(f"stand-alone C={C} {shape} {precision}", "nested", precision, alone[shape][0],
                       oracle_logits("nested", C, shape, case("nested", C, shape)[0]), oracle)
    print(f"C={C} {precision}: fused against stand-alone head, max|dlogit| = {worst:.3e} (bar {HEAD_UNFUSED_BAR[precision]})")
    assert HEAD_UNFUSED_BAR[precision] is not None and worst < HEAD_UNFUSED_BAR[precision]
    assert m.status() == 0


# ----------------------------------------------------------------------------- d. exact ties
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C", CLASS_COUNTS[1:])
@pytest.mark.parametrize("arch", ["nested", "simple"])
def test_exact_ties(arch, C, precision, torch_cuda, engines, inputs, syn):
    """Row and bias b are bit copies of row and bias a (the rows winning most and second most pixels), rotated through every
    index so that the original comes first and the copy comes first: equal logit and probability planes, the earlier class wins
    (np.argmax), on at least 25 % of the pixels.  Fused heads, and for NestedUNet the stand-alone head as well."""
    torch = torch_cuda
    m = engines(arch, C, precision)
    a, b = tie_pair(arch, C, shapes_of(arch)[0])
    tied = syn.tie_head(case(arch, C, shapes_of(arch)[0])[0], a, b)
    for j in range(C):
        lo, hi = sorted(((a + j) % C, (b + j) % C))
        m.load_state_dict(syn.rotate_head(tied, j), strict=True)
        for shape in shapes_of(arch):
            for keep in (False, True) if arch == "nested" else (False,):
                try:
                    check_tie(run(torch, m, inputs(arch, shape), keep=keep), C, lo, hi)
                except AssertionError as err:
                    raise AssertionError(f"{arch} C={C} {precision} {shape} rotation {j} pair ({lo}, {hi}) stand-alone={keep}: {err}") from None
    m.debug_keep_intermediates(False)


# ----------------------------------------------------------------------------- e. constant logits
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C", CLASS_COUNTS)
@pytest.mark.parametrize("arch", ["nested", "simple"])
def test_constant_logits(arch, C, precision, torch_cuda, engines, inputs, syn):
    """Head weights +0.0: every logit is its class's bias exactly, the mask the first maximal index, the probabilities the
    float64 softmax within 1e-6 -- 1 / C exactly for equal biases ('/' is correctly rounded in this build: no fast-math flag,
    hipcc's default), exactly 1 and 0 for +80 against -80, and never a NaN from the -inf slots c >= C.  On the three paths that
    produce `out`: fused wave-specialised, fused lock-step, stand-alone."""
    torch = torch_cuda
    m = engines(arch, C, precision)
    sd = case(arch, C, shapes_of(arch)[0])[0]
    shape = shapes_of(arch)[-1]
    for tag, biases in constant_bias_cases(C):
        m.load_state_dict(syn.constant_head(sd, biases), strict=True)
        for keep in (False, True) if arch == "nested" else (False,):
            try:
                check_constant(run(torch, m, inputs(arch, shape), keep=keep), C, tag, biases)
            except AssertionError as err:
                raise AssertionError(f"{arch} C={C} {precision} {tag} stand-alone={keep}: {err}") from None
    m.debug_keep_intermediates(False)
    assert m.status() == 0


# ----------------------------------------------------------------------------- f. deep supervision and pruned outputs
@pytest.mark.parametrize("precision", ["exact", "exact8"])
@pytest.mark.parametrize("C", DS_CLASS_COUNTS)
def test_deep_supervision_outputs(C, precision, torch_cuda, engines, inputs, syn, oracle):
    torch = torch_cuda
    B, H, W = DS_SHAPE
    sd, _, x = case("nested", C, DS_SHAPE)
    xt = inputs("nested", DS_SHAPE)
    m = engines("nested", C, precision)
    m.debug_keep_intermediates(False)
    m.load_state_dict(sd, strict=True)
    outs = [t.cpu().numpy() for t in m.forward_deep_supervision(xt)]
    refs = oracle_ds(oracle, sd, x, H, W)
    tol = DS_EXACT_TOL if precision == "exact" else DS_LOGIT_TOL
    for k in range(4):
        res = run(torch, m, xt, output=k)
        assert np.array_equal(bits(res["logits"]), bits(outs[k])), k                   # the pruned pass computes entry k's bits
        check_outputs(res, C)                                                           # its mask is np.argmax of those logits
        err = float(np.abs(outs[k] - refs[k]).max())
        flips = unexplained_flips(res["mask"], oracle.masks_from_logits(refs[k])[0], oracle.top2_margin(refs[k]), err)
        print(f"C={C} {precision} out{k}: max|dlogit|={err:.3e} unexplained mask flips={flips}")
        assert err <= tol and flips == 0, (k, err, flips)
    if C > 1:
        m.load_state_dict(syn.rotate_head(sd, 1), strict=True)
        for k, t in enumerate(m.forward_deep_supervision(xt)):
            assert np.array_equal(bits(t.cpu().numpy()), bits(np.roll(outs[k], 1, axis=1))), k
    assert m.status() == 0


# ----------------------------------------------------------------------------- g. class rules
@pytest.mark.parametrize("precision", ["exact", "exact8"])
@pytest.mark.parametrize("C", RULE_CLASS_COUNTS)
def test_class_rules_above_three_classes(C, precision, torch_cuda, engines, inputs, syn, oracle):
    """The rules see classes 0 .. 2 only (apply_rule; oracle: probs[..., :3]); in the second rotation class 3 is the overall
    argmax of most pixels.  A pixel may differ from the oracle's only within twice the probability error of a decision
    boundary, and at most 0.5 % of the pixels are that near (test_logit_scale's bars)."""
    torch = torch_cuda
    sd, _, _ = case("nested", C, RULE_SHAPE)
    xt = inputs("nested", RULE_SHAPE)
    m = engines("nested", C, precision)
    m.debug_keep_intermediates(False)
    js = rule_rotations(C)
    for j in js:
        rot = syn.rotate_head(sd, j)
        m.load_state_dict(rot, strict=True)
        ref = oracle_logits("nested", C, RULE_SHAPE, rot)
        p64 = softmax64(ref)
        res = run(torch, m, xt)
        if j == js[1]:
            assert float((res["mask"] == 3).mean()) > 0.5
        perr = float(np.abs(res["probs"] - p64).max())
        for rule, params in RULES:
            cable, tape = m.segment_thresholded(xt, rule=rule, **params)
            torch.cuda.synchronize()
            rc, rt, _ = oracle.rule_masks_from_logits(ref, rule, **params)
            diff = (cable.cpu().numpy() != rc) | (tape.cpu().numpy() != rt)
            near = boundary_distance(p64, rule, params) <= 2 * perr
            print(f"C={C} {precision} rotation {j} {rule}: {int(diff.sum())} pixels differ, {float(near.mean()):.3%} within 2 x {perr:.1e} of a boundary, "
                  f"cable {int(rc.sum())} tape {int(rt.sum())} pixels")
            assert not (diff & ~near).any(), (j, rule)
            assert float(near.mean()) <= NEAR_CAP, (j, rule)


@pytest.mark.parametrize("C", [1, 2])
def test_class_rules_need_three_classes(C, torch_cuda, engines, inputs):
    m = engines("nested", C, "exact")
    m.load_state_dict(case("nested", C, RULE_SHAPE)[0], strict=True)
    with pytest.raises(RuntimeError, match="class rules need num_classes >= 3"):
        m.segment_thresholded(inputs("nested", RULE_SHAPE))
    assert m.segment(inputs("nested", RULE_SHAPE)).shape == RULE_SHAPE
