"""CPU side of the value-range sweep (tests/test_gpu_value_range.py is the device side).

Every parity fixture of the suite is one operating point: stored activations around 1, logits in +-3.  The engine stores
activations as fp16 planes (include/unetpp.h "Value range"), which have a window; the fp32 reference (src/models/unetpp.py:23-26:
conv -> BatchNorm -> ReLU) does not care where in it a tensor sits, because a block's (gamma, beta) and its consumers' weights
trade any power of two.  Checked here, without a GPU:

  * `synthetic.rescale_state_dict` / `rescale_simple_state_dict` move ONE tensor by 2^k and leave every reference output
    bitwise unchanged (deep-supervision outputs included), while the tensor itself is exactly 2^k times the original.  This
    is what licenses the device assertions: the expected logits of a rescaled checkpoint are the unscaled ones.
  * `oracle/exact_emulation.py` (float64 emulation of DESIGN.md §3's `exact` arithmetic, the predicted behaviour, not the code
    under test): its error against the oracle per site and k is printed, and the WINDOW is derived from it -- the k down to
    which the documented arithmetic stays within half of the bar the suite holds `exact` to on small fixtures (2e-5, so 1e-5).
  * negative controls of the device tests, run against the emulation (see the docstrings there).
"""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_ds_host import DS

sys.path.insert(0, os.path.join(ROOT, "oracle"))

KS = (-18, -10, -6, 6, 12)
NB = (32, 64, 128, 256, 512)
F16_MAX = 65504.0
EXACT_SMALL_BAR = 2e-5                 # what tests/test_range_status.py and test_gpu_exact8.py hold `exact` to at sizes like these
WINDOW_BAR = EXACT_SMALL_BAR / 2       # the emulation must leave the device half of it
NORTH_STAR = 1e-3
SWEEP = (-18, -16, -14, -12, -10, -8, -6, -3, 0, 3, 6)


def nested_case(C=3, B=1, H=64, W=64):
    from unet_amd import synthetic as syn
    sd = syn.make_state_dict(C, 3, True, 2)
    x = syn.frames_to_chw_f32(syn.make_frames_u8(B, H, W, "smooth", 7))
    return sd, x


def reference_tensors(oracle, sd, x):
    """oracle.torch_forward plus the tensors it does not hand out: every block's inner tensor 'x..a' (relu(bn1(conv1(.))) of the
    same ATen ops on the oracle's own nodes, so the same bits) and the pooled 'x..p'.  Returns (logits, {name: array})."""
    import torch
    import torch.nn.functional as F
    logits, t = oracle.torch_forward(sd, x, return_intermediates=True)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    up = lambda a: F.interpolate(a, scale_factor=2, mode="bilinear", align_corners=True)
    out = dict(t)
    with torch.no_grad():
        src = {"x0_0": T(x).float()}
        for l in range(4):
            p = F.max_pool2d(T(t[f"x{l}_0"]), 2, 2)
            out[f"x{l}_0p"] = p.numpy()
            src[f"x{l + 1}_0"] = p
        low = "x4_0"
        for l in (3, 2, 1, 0):
            src[f"x{l}_{4 - l}"] = torch.cat([T(t[f"x{l}_0"]), up(T(t[low]))], 1)
            low = f"x{l}_{4 - l}"
        for node, inp in src.items():
            blk = "conv" + node[1:]
            a = F.conv2d(inp, T(sd[f"{blk}.conv1.weight"]), T(sd[f"{blk}.conv1.bias"]), padding=1)
            a = F.batch_norm(a, T(sd[f"{blk}.bn1.running_mean"]), T(sd[f"{blk}.bn1.running_var"]), T(sd[f"{blk}.bn1.weight"]),
                             T(sd[f"{blk}.bn1.bias"]), False, 0.1, oracle.BN_EPS)
            out[node + "a"] = F.relu(a).numpy()
    return logits, out


def ds_outputs(sd, t, H, W):
    """[out1, out2, out3] of the reference's deep-supervision list, as tests/test_ds_host.py restates them"""
    import torch
    import torch.nn.functional as F
    outs = []
    for head, node, _ in DS:
        low = F.conv2d(torch.from_numpy(t[node]), torch.from_numpy(sd[head + ".weight"]), torch.from_numpy(sd[head + ".bias"]))
        outs.append(F.interpolate(low, size=(H, W), mode="bilinear", align_corners=True).numpy())
    return outs


def k_hi(peak: float) -> int:
    """the largest k that keeps a tensor peaking at `peak` below 0.9 x 65504 (it then peaks at 29,000 ... 59,000)"""
    return int(np.floor(np.log2(0.9 * F16_MAX / peak)))


@functools.lru_cache(maxsize=None)
def emulated_error(site: str, k: int, C=3, B=1, H=64, W=64, what="exact"):
    """max |emulated logits - oracle logits| of the checkpoint rescaled at (site, k)"""
    import exact8_emulation as em8
    import exact_emulation as em
    import unetpp_oracle as oracle
    from unet_amd import synthetic as syn
    sd, x = nested_case(C, B, H, W)
    rs = syn.rescale_state_dict(sd, site, k)
    ref = oracle.torch_forward(rs, x)
    lg = em.exact_forward(rs, x) if what == "exact" else em8.exact8_forward(rs, x)
    return float(np.abs(lg - ref).max())


@functools.lru_cache(maxsize=None)
def window_low(site: str) -> int:
    """the smallest k of the sweep from which the emulation of `exact` stays within WINDOW_BAR all the way up to k = 0 (64x64
    case of this file).  Computed, not typed in; the device tests take their window from here."""
    lo = 0
    for k in sorted((k for k in SWEEP if k < 0), reverse=True):
        if emulated_error(site, k) > WINDOW_BAR:
            break
        lo = k
    return lo


@functools.lru_cache(maxsize=None)
def below_window(site: str):
    """the k of the sweep below the window, down to (and including) the first at which the emulation itself reaches 1e-3"""
    ks = []
    for k in sorted((k for k in SWEEP if k < window_low(site)), reverse=True):
        ks.append(k)
        if emulated_error(site, k) >= NORTH_STAR:
            break
    return tuple(ks)


# ----------------------------------------------------------------------------- A. the rescaling tool
def test_nested_rescale_leaves_the_reference_bitwise_unchanged(syn, oracle):
    import torch
    torch.set_num_threads(8)
    sd, x = nested_case()
    ref, t = reference_tensors(oracle, sd, x)
    ref_ds = ds_outputs(sd, t, 64, 64)
    for site in syn.NESTED_SITES:
        for k in KS:
            rs = syn.rescale_state_dict(sd, site, k)
            assert all(v.dtype == sd[n].dtype for n, v in rs.items())
            lg, tt = reference_tensors(oracle, rs, x)
            assert np.array_equal(lg, ref), (site, k, float(np.abs(lg - ref).max()))
            for a, b in zip(ds_outputs(rs, tt, 64, 64), ref_ds):
                assert np.array_equal(a, b), (site, k, "deep-supervision output")
            assert np.array_equal(tt[site], t[site] * np.float32(2.0 ** k)), (site, k)
            for name in t:                                   # its pooled copy moves with it, nothing else does
                if name not in (site, site + "p"):
                    assert np.array_equal(tt[name], t[name]), (site, k, name)
            if site + "p" in t:
                assert np.array_equal(tt[site + "p"], t[site + "p"] * np.float32(2.0 ** k)), (site, k)
    before = syn.make_state_dict(3, 3, True, 2)
    assert all(np.array_equal(before[n], sd[n]) for n in sd)          # the input dict is not touched


def test_nested_rescale_without_ds_heads_and_bad_sites(syn, oracle):
    sd = {n: v for n, v in nested_case()[0].items() if not n.startswith("ds")}
    x = nested_case()[1]
    ref = oracle.torch_forward(sd, x)
    for site in ("x3_1", "x2_2", "x1_3"):
        assert np.array_equal(oracle.torch_forward(syn.rescale_state_dict(sd, site, -10), x), ref)
    for bad in ("x0_1", "x5_0", "enc1", "x0_0p", ""):
        with pytest.raises(ValueError):
            syn.rescale_state_dict(sd, bad, 1)
    with pytest.raises(ValueError):
        syn.rescale_state_dict(sd, "x0_0", 200)


def test_simple_rescale_leaves_the_reference_bitwise_unchanged(syn, oracle):
    import torch
    torch.set_num_threads(8)
    sd = syn.make_simple_state_dict(7, 3, 0)
    x = syn.frames_to_chw_f32(syn.make_frames_u8(1, 64, 64, "smooth", 7))
    ref, t = oracle.simple_unet_torch_forward(sd, x, return_intermediates=True)
    for site in syn.SIMPLE_SITES:
        for k in KS:
            lg, tt = oracle.simple_unet_torch_forward(syn.rescale_simple_state_dict(sd, site, k), x, return_intermediates=True)
            assert np.array_equal(lg, ref), (site, k, float(np.abs(lg - ref).max()))
            for name in t:                                   # the oracle hands out enc1..4 and dec3..1
                want = t[name] * np.float32(2.0 ** k) if name == site else t[name]
                assert np.array_equal(tt[name], want), (site, k, name)
    with pytest.raises(ValueError):
        syn.rescale_simple_state_dict(sd, "x0_0", 1)


@pytest.mark.parametrize("C", [3, 7])
def test_logit_site_scales_the_logits_exactly(C, syn, oracle):
    sd, x = nested_case(C)
    ref = oracle.torch_forward(sd, x)
    for k in KS + (2, 4):
        lg = oracle.torch_forward(syn.rescale_state_dict(sd, "logits", k), x)
        assert np.array_equal(lg, ref * np.float32(2.0 ** k)), k
    ss = syn.make_simple_state_dict(C, 3, 0)
    ref = oracle.simple_unet_torch_forward(ss, x)
    assert np.array_equal(oracle.simple_unet_torch_forward(syn.rescale_simple_state_dict(ss, "logits", 4), x), ref * np.float32(16))


# ----------------------------------------------------------------------------- B. the emulation of `exact` and the window
def test_emulation_error_table_and_window(syn, oracle):
    """Prints, per site and k, the emulated `exact` error against the oracle and derives the window from it.  What is asserted
    is only what the documented arithmetic promises regardless of the figures: at the usual scale and above it the emulation is
    well inside the bar, the error grows monotonically (within a factor) once the lo plane goes subnormal, and every site that
    is split into planes has a finite window.  x0_4 is never split (the head reads conv0_4.conv2's fp32 registers): flat."""
    import torch
    torch.set_num_threads(8)
    print("\nemulated `exact` max |dlogit| vs the oracle, 3-class 1x64x64, weights seed 2, frame smooth/7")
    print("site    peak   " + "".join(f"{('2^%d' % k):>9}" for k in SWEEP) + "   window from")
    _, t = reference_tensors(oracle, *nested_case())
    for site in syn.NESTED_SITES:
        errs = [emulated_error(site, k) for k in SWEEP]
        print(f"{site:<7}{float(t[site].max()):5.2f}   " + "".join(f"{e:9.1e}" for e in errs) + f"   2^{window_low(site)}"
              f"   (below it, tested down to 2^{min(below_window(site), default=window_low(site))})")
        assert all(e < WINDOW_BAR for k, e in zip(SWEEP, errs) if k >= 0), site
        if site == "x0_4":
            assert max(errs) < WINDOW_BAR and window_low(site) == min(SWEEP)
            continue
        assert -14 < window_low(site) <= -6, (site, window_low(site))       # lo is subnormal below 0.25: a window must exist
        assert errs[0] > NORTH_STAR                                          # and at 2^-18 the arithmetic has left the north-star bar
        low = [e for k, e in zip(SWEEP, errs) if k <= -10]
        assert all(a > 1.5 * b for a, b in zip(low, low[1:])), (site, low)   # every two binades cost about 4x
    print(f"window bar {WINDOW_BAR:.0e} (half of the {EXACT_SMALL_BAR:.0e} the suite holds `exact` to on small fixtures)")


def test_emulation_at_the_top_of_the_window(syn, oracle):
    """k = k_hi (the tensor peaks at 29,000 ... 59,000): both emulations stay at their usual error -- the consumer's 2^-14 times
    smaller weight slice beside an unscaled slice costs nothing visible -- so the device bars of C.1 are reachable there."""
    _, t = reference_tensors(oracle, *nested_case())
    for site in ("x0_0", "x1_0a", "x4_0", "x2_2", "x1_3a"):
        k = k_hi(float(t[site].max()))
        e, e8 = emulated_error(site, k), emulated_error(site, k, what="exact8")
        print(f"{site}: k_hi = {k}, peak {float(t[site].max()) * 2.0 ** k:.0f}: exact {e:.2e}, exact8 {e8:.2e}")
        assert 29000 <= float(t[site].max()) * 2.0 ** k <= 59000
        assert e < WINDOW_BAR and e8 < NORTH_STAR / 2


def test_negative_controls_against_the_emulation(syn, oracle):
    """The device checks of tests/test_gpu_value_range.py, applied to emulations that are wrong in one documented way: each
    must fail its check (and the right emulation passes it)."""
    import exact_emulation as em
    sd, x = nested_case()
    _, t = reference_tensors(oracle, sd, x)
    site = "x2_2"
    k = k_hi(float(t[site].max()))
    rs = syn.rescale_state_dict(sd, site, k)
    ref, tt = reference_tensors(oracle, rs, x)
    peak = float(tt[site].max())

    def c1(**knobs):          # C.1: logits within 2e-5, the node within 2e-5 of its peak
        lg, nodes = em.exact_forward(rs, x, return_nodes=True, **knobs)
        return float(np.abs(lg - ref).max()) < EXACT_SMALL_BAR and float(np.abs(nodes[site] - tt[site]).max()) < EXACT_SMALL_BAR * peak
    assert c1()
    assert not c1(drop_lo=(site,))
    assert not c1(clamp=32768.0)

    over = syn.rescale_state_dict(sd, "x1_0", k_hi(float(t["x1_0"].max())) + 2)
    _, to = reference_tensors(oracle, over, x)
    assert float(to["x1_0"].max()) > F16_MAX

    def c3(**knobs):          # C.3 on the pooled tensor: 65504 where the oracle is above, close to it where it is below
        _, nodes = em.exact_forward(over, x, return_nodes=True, **knobs)
        return clamp_check(nodes["x1_0p"], to["x1_0p"]) is None
    assert c3()
    assert not c3(pool_unclamped=True)


def clamp_check(got, want, margin=1e-4, tol=EXACT_SMALL_BAR):
    """C.3's value check: exactly +-65504 wherever the reference is beyond 65504 (1 + margin), within tol x 65504 of it wherever
    it is inside 65504 (1 - margin), finite and inside the range everywhere.  Returns None or a description of the failure."""
    if not np.isfinite(got).all():
        return "non-finite values"
    above, below = np.abs(want) > F16_MAX * (1 + margin), np.abs(want) < F16_MAX * (1 - margin)
    wrong = got[above] != np.sign(want[above]) * np.float32(F16_MAX)
    if wrong.any():
        return f"{int(wrong.sum())} of {int(above.sum())} elements over the limit are not +-65504"
    d = float(np.abs(got[below] - want[below]).max()) if below.any() else 0.0
    if d > tol * F16_MAX:
        return f"unclamped elements off by {d:.3e}"
    if float(np.abs(got).max()) > F16_MAX:
        return "a value beyond 65504"
    return None


# ----------------------------------------------------------------------------- C.4: the class rules' thresholds at scaled logits
RULES = (("thresholded_argmax", dict(t_cable=0.45, t_tape=0.50, bg_margin=0.15)),
         ("strict_bg_check", dict(t_cable=0.6, t_tape=0.65, bg_margin=0.4)),
         # `exclusive` makes six comparisons per pixel; at the reference scripts' defaults (0.55 / 0.60 / 0.20 / 0.10) up to 0.9 %
         # of the pixels of these cases sit within exact8's probability error of one of them: thresholds moved, cap kept
         ("exclusive", dict(t_cable=0.75, t_tape=0.80, bg_margin=0.40, ct_margin=0.40)))
LOGIT_SHAPES = {"64x96": (2, 64, 96), "1x512x512": (1, 512, 512)}
LOGIT_CASES = [(3, "64x96", k) for k in (0, 2, 4, 6)] + [(7, "64x96", k) for k in (0, 2, 4, 6)] + [(3, "1x512x512", 4)]


def boundary_distance(p, rule, params):
    """distance of every pixel's probabilities [B,C,H,W] to the nearest decision boundary of one class rule: the comparisons
    oracle.thresholded_argmax_np, strict_threshold_with_bg_check_np or exclusive_threshold_np makes, each as |lhs - rhs|"""
    p0, p1, p2 = p[:, 0], p[:, 1], p[:, 2]
    tc, tt, bgm = params["t_cable"], params["t_tape"], params["bg_margin"]
    terms = [np.abs(p1 - tc), np.abs(p2 - tt)]
    if rule == "exclusive":
        ctm = params["ct_margin"]
        terms += [np.abs(p1 - p0 - bgm), np.abs(p2 - p0 - bgm), np.abs(p1 - p2 - ctm), np.abs(p2 - p1 - ctm)]
    else:
        top = np.sort(p[:, :3], axis=1)      # the winner changes only where the two largest of (bg, cable, tape) are close -- where
        tie = top[:, 2] - top[:, 1]          # exp saturates the two losers are both 0, which is no boundary, nor is a tie between
        terms.append(np.maximum(tie, min(tc, tt) - top[:, 2]))      # three that are all below every threshold (7 classes)
        terms += [np.abs(p0 - bgm)] if rule == "strict_bg_check" else [np.abs(p1 - p0 - bgm), np.abs(p2 - p0 - bgm)]
    return np.minimum.reduce(terms)


def softmax64(logits):
    z = logits.astype(np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def test_rule_thresholds_leave_few_pixels_near_a_boundary(syn, oracle):
    """The device test lets the class rules differ from the oracle's only at pixels whose probability is within twice the
    probability error of a decision boundary, and caps those at 0.5 % of the pixels.  The oracle's own logits must satisfy that
    cap with the fp32-versus-float64 softmax difference in place of the device's error, for every case of the device test."""
    import torch
    torch.set_num_threads(8)
    for C, shape_tag, k in LOGIT_CASES:
        sd, x = nested_case(C, *LOGIT_SHAPES[shape_tag])
        ref = oracle.torch_forward(syn.rescale_state_dict(sd, "logits", k), x)
        p64 = softmax64(ref)
        for rule, params in RULES:
            _, _, p32 = oracle.rule_masks_from_logits(ref, rule, **params)
            d = float(np.abs(np.transpose(p32, (0, 3, 1, 2)) - p64).max())
            near = float((boundary_distance(p64, rule, params) <= 2 * d).mean())
            print(f"C={C} {shape_tag} logits x 2^{k} (largest {float(np.abs(ref).max()):.1f}) {rule}: softmax fp32 vs float64 {d:.1e}, "
                  f"{near:.4%} of the pixels within twice that of a boundary")
            assert d < 1e-6 and near <= 0.005, (C, shape_tag, k, rule)
