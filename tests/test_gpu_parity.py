"""Parity of the HIP path (through the C ABI) against the oracle and the committed golden vectors.
Run on the GPU box:  python -m pytest tests -m gpu"""
import hashlib

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3     # north_star: logits within 1e-3 (fp32)
EXACT_TOL = 2e-5     # what `exact` is held to on small fixtures and at 512x512 (fp32-class)
FAST_TOL = 5e-2      # `fast` (plain fp16) at 512x512
HEAD_UNFUSED_TOL = 2e-6                       # `exact`: the fused head against head_generic_kernel on the stored x0_4
SIMPLE_EXACT_TOL, SIMPLE_FAST_TOL = 5e-5, 6e-2   # SimpleUNet
NODES = ("x0_0", "x1_0", "x2_0", "x3_0", "x4_0", "x3_1", "x2_2", "x1_3", "x0_4")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


def make_model(C, ds, wseed, precision, syn, max_batch, hw, micro_batch=0, streams=1):
    from unet_amd.nested_unet import NestedUNet
    sd = syn.make_state_dict(C, 3, ds, wseed)
    m = NestedUNet(C, deep_supervision=ds, precision=precision, max_batch=max_batch, max_hw=hw,
                   micro_batch=micro_batch, streams=streams).to("cuda:0")
    m.load_state_dict(sd, strict=True)
    return m.eval(), sd


def report(logits, mask, ref_logits, ref_mask, oracle):
    err = float(np.abs(logits - ref_logits).max())
    margin = oracle.top2_margin(ref_logits)
    flips = mask != ref_mask
    unexplained = flips & (margin > 2 * err + 1e-7)
    return err, int(flips.sum()), int(unexplained.sum())


@pytest.mark.parametrize("tag", ["s_c3_32x32", "s_c3_64x64", "s_c7_48x80", "s_c3_128x96"])
def test_exact_matches_golden_small(tag, torch_cuda, syn, oracle):
    torch = torch_cuda
    g = load_golden(tag)
    B, H, W, C = int(g["B"]), int(g["H"]), int(g["W"]), int(g["num_classes"])
    frames = syn.make_frames_u8(B, H, W, str(g["kind"]), int(g["fseed"]))
    assert hashlib.sha256(frames.tobytes()).hexdigest() == str(g["frames_sha"])
    model, _ = make_model(C, bool(g["deep_supervision"]), int(g["wseed"]), "exact", syn, B, (H, W))
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    logits = model(x)
    mask, cable, tape = model.segment(x, return_class_masks=True)
    torch.cuda.synchronize()
    err, flips, unexplained = report(logits.cpu().numpy(), mask.cpu().numpy(), g["logits"], g["mask"], oracle)
    print(f"{tag}: max|dlogit|={err:.3e} flips={flips}")
    if tag == "s_c3_32x32":                 # layer-by-layer against the reference's intermediates
        model.debug_keep_intermediates(True)          # unfused head path: materialises x0_4
        logits_unfused = model(x)
        torch.cuda.synchronize()
        assert float((logits_unfused - logits).abs().max()) < HEAD_UNFUSED_TOL     # fused and unfused heads agree
        for name in NODES:
            got = model.debug_activation(name, B, H, W)
            np.testing.assert_allclose(got, g["t_" + name], rtol=0, atol=2e-5, err_msg=name)
    assert err < EXACT_TOL                  # exact mode is fp32-class, far inside the 1e-3 bar
    assert flips == 0                       # bit-exact masks on the committed fixtures
    assert np.array_equal(cable.cpu().numpy(), g["mask_cable"]) and np.array_equal(tape.cpu().numpy(), g["mask_tape"])


def test_u8_bgr_input_equals_f32_input(torch_cuda, syn):
    torch = torch_cuda
    frames = syn.make_frames_u8(2, 48, 64, "uniform", 3)
    model, _ = make_model(3, True, 2, "exact", syn, 2, (48, 64))
    a = model(torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda())
    m_u8, l_u8 = model.segment(torch.from_numpy(frames).cuda(), return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(a, l_u8)             # same arithmetic: bitwise equal
    assert torch.equal(m_u8, a.argmax(1).to(torch.uint8))


def test_full_size_512_exact_and_fast(torch_cuda, syn, oracle):
    torch = torch_cuda
    g = load_golden("b_c3_512x512")
    kinds = [str(k) for k in g["kinds"]]
    B = int(g["B"])
    frames = np.stack([syn.make_frame_u8(512, 512, i, kinds[i % len(kinds)], int(g["fseed"])) for i in range(B)])
    assert hashlib.sha256(frames.tobytes()).hexdigest() == str(g["frames_sha"])
    x = syn.frames_to_chw_f32(frames)
    sd = syn.make_state_dict(3, 3, True, int(g["wseed"]))
    ref = oracle.torch_forward(sd, x)                      # oracle on this host's cores
    ref_mask, _, _ = oracle.masks_from_logits(ref)
    ties = {tuple(t) for t in g["tie_idx"].tolist()}
    assert all(tuple(d) in ties for d in np.argwhere(ref_mask != g["mask"]).tolist())
    xt = torch.from_numpy(x).cuda()
    for precision, tol in (("exact", EXACT_TOL), ("fast", FAST_TOL)):
        model, _ = make_model(3, True, int(g["wseed"]), precision, syn, B, (512, 512))
        mask, logits = model.segment(xt, return_logits=True)
        torch.cuda.synchronize()
        lg = logits.cpu().numpy()
        err, flips, unexplained = report(lg, mask.cpu().numpy(), ref, ref_mask, oracle)
        sub = float(np.abs(lg[:, :, ::8, ::8] - g["logits_sub8"]).max())
        print(f"512x512 {precision}: max|dlogit|={err:.3e} (vs golden sub8 {sub:.3e}) "
              f"flips={flips}/{mask.numel()} unexplained={unexplained}")
        assert err < tol and sub < tol
        assert unexplained == 0
        if precision == "exact":
            assert err < LOGIT_TOL
            gold_flips = np.argwhere(mask.cpu().numpy() != g["mask"])
            assert all(tuple(d) in ties for d in gold_flips.tolist())     # only listed near-tie pixels may differ
            assert len(gold_flips) <= 4
        del model


def test_7class_448x800(torch_cuda, syn, oracle):
    torch = torch_cuda
    g = load_golden("b_c7_448x800")
    frames = np.stack([syn.make_frame_u8(448, 800, 0, "smooth", int(g["fseed"]))])
    assert hashlib.sha256(frames.tobytes()).hexdigest() == str(g["frames_sha"])
    model, _ = make_model(7, False, int(g["wseed"]), "exact", syn, 1, (448, 800))
    mask, logits = model.segment(torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda(), return_logits=True)
    torch.cuda.synchronize()
    sub = float(np.abs(logits.cpu().numpy()[:, :, ::8, ::8] - g["logits_sub8"]).max())
    ties = {tuple(t) for t in g["tie_idx"].tolist()}
    diff = np.argwhere(mask.cpu().numpy() != g["mask"])
    print(f"7c 448x800: sub8 err={sub:.3e} flips={len(diff)}")
    assert sub < 2e-5
    assert all(tuple(d) in ties for d in diff.tolist()) and len(diff) <= 4


def test_batch_and_microbatch_invariance(torch_cuda, syn, monkeypatch):
    """Micro-batching, concurrent passes and a frame's position in the batch never change a bit -- under ONE launch plan.
    (The split-K plan of small launches depends on the frames per pass: switched off here, its own test follows.)"""
    torch = torch_cuda
    monkeypatch.setenv("UNETPP_KSPLIT", "1")
    frames = syn.make_frames_u8(5, 64, 64, "smooth", 21)
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    full, _ = make_model(3, True, 2, "exact", syn, 5, (64, 64))
    micro, _ = make_model(3, True, 2, "exact", syn, 5, (64, 64), micro_batch=2)
    multi, _ = make_model(3, True, 2, "exact", syn, 5, (64, 64), micro_batch=1, streams=3)
    a = full(x); b = micro(x); c = full(x[3:4]); d = multi(x); d2 = multi(x)
    torch.cuda.synchronize()
    assert torch.equal(a, b)                 # micro-batching never changes results
    assert torch.equal(a, d) and torch.equal(a, d2)   # nor do concurrent passes on internal streams
    assert torch.equal(a[3:4], c)            # a frame's result does not depend on its batch


def test_split_k_plan_changes_rounding_only(torch_cuda, syn, oracle, monkeypatch):
    """Small launches share a tile's K-chunks among several workgroups (conv3x3_ws.h, split-K): the partial sums are added in
    a fixed order, so a plan is deterministic, but two plans (different frames per pass, or UNETPP_KSPLIT=1) add in different
    orders.  512x512: batch 1 splits levels 3-4, batch 4 does not.  Same plan: bitwise; different plans: fp32 rounding only,
    both against the oracle at the exact-mode bar."""
    torch = torch_cuda
    frames = syn.make_frames_u8(4, 512, 512, "smooth", 33)
    x = syn.frames_to_chw_f32(frames)
    xt = torch.from_numpy(x).cuda()
    model, sd = make_model(3, True, 2, "exact", syn, 4, (512, 512))
    m4, l4 = model.segment(xt, return_logits=True)
    m1, l1 = model.segment(xt[2:3], return_logits=True)
    m1b, l1b = model.segment(xt[2:3], return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(l1, l1b) and torch.equal(m1, m1b)                 # a plan reproduces itself bit for bit
    monkeypatch.setenv("UNETPP_KSPLIT", "1")
    plain, _ = make_model(3, True, 2, "exact", syn, 4, (512, 512))
    mp, lp = plain.segment(xt[2:3], return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(lp, l4[2:3]) and torch.equal(mp, m4[2:3])         # no split in either: the same plan, the same bits
    d = float((l1 - l4[2:3]).abs().max())
    print(f"split-K plan vs unsplit plan: max|dlogit|={d:.3e}, mask pixels differing {int((m1 != m4[2:3]).sum())}")
    assert 0 < d < 5e-6                                                  # the split did happen, and moved roundings only
    ref = oracle.torch_forward(sd, x[2:3])
    ref_mask, _, _ = oracle.masks_from_logits(ref)
    for name, lg, mk in (("split", l1, m1), ("unsplit", l4[2:3], m4[2:3])):
        err, flips, unexplained = report(lg.cpu().numpy(), mk.cpu().numpy(), ref, ref_mask, oracle)
        print(f"  {name}: max|dlogit|={err:.3e} flips={flips}")
        assert err < 2e-5 and unexplained == 0


def test_errors(torch_cuda, syn):
    torch = torch_cuda
    from unet_amd.nested_unet import NestedUNet
    model, sd = make_model(3, True, 2, "exact", syn, 1, (32, 32))
    with pytest.raises(RuntimeError, match="multiples of 16"):
        model(torch.zeros(1, 3, 100, 100, device="cuda"))
    with pytest.raises(RuntimeError):
        model(torch.zeros(1, 3, 32, 32))                     # CPU tensor: no fallback
    with pytest.raises(RuntimeError):
        NestedUNet(3).to("cpu")
    m2 = NestedUNet(3).to("cuda:0")
    with pytest.raises(RuntimeError, match="load_state_dict"):
        m2(torch.zeros(1, 3, 32, 32, device="cuda"))
    bad = dict(sd); bad.pop("final.bias")
    with pytest.raises(RuntimeError, match="Missing key"):
        m2.load_state_dict(bad, strict=True)
    sd7 = syn.make_state_dict(7, 3, True, 0)
    with pytest.raises(RuntimeError, match="size mismatch"):
        m2.load_state_dict(sd7, strict=True)


@pytest.mark.parametrize("C,B,H,W", [(3, 1, 16, 16), (3, 3, 16, 80), (7, 2, 80, 16), (3, 2, 112, 144), (7, 1, 32, 224),
                                     # every class count the reference's callers construct (2, 3, 4, 6, 7) and the limits 1, 8
                                     (1, 1, 16, 32), (2, 1, 32, 48), (4, 2, 48, 32), (6, 1, 32, 64), (8, 1, 16, 48),
                                     # one tile row / one tile column of maximal length
                                     (3, 1, 16, 4096), (3, 1, 4096, 16)])
def test_ragged_shapes_against_oracle(C, B, H, W, torch_cuda, syn, oracle):
    """Minimum size, single row/column of tiles, widths that are not multiples of the 32-pixel tile
    (80 = 2.5 tiles, 144 = 4.5), heights that are not multiples of the 16-row tile: oracle on the host."""
    torch = torch_cuda
    ds = C == 3
    frames = syn.make_frames_u8(B, H, W, "uniform", 100 + H + W)
    x = syn.frames_to_chw_f32(frames)
    model, sd = make_model(C, ds, 2, "exact", syn, B, (H, W))
    ref = oracle.torch_forward(sd, x)
    ref_mask, ref_cable, ref_tape = oracle.masks_from_logits(ref)
    mask, cable, tape, logits = model.segment(torch.from_numpy(frames).cuda(), return_logits=True, return_class_masks=True)
    torch.cuda.synchronize()
    err, flips, unexplained = report(logits.cpu().numpy(), mask.cpu().numpy(), ref, ref_mask, oracle)
    print(f"C={C} {B}x{H}x{W}: max|dlogit|={err:.3e} flips={flips}")
    # 2e-5 everywhere except the 4096-long strips, where the CPU library itself switches algorithm (4e-5); gate = 1e-3
    assert err < (1e-4 if max(H, W) >= 4096 else 2e-5) and unexplained == 0
    agree = mask.cpu().numpy() == ref_mask
    assert np.array_equal(cable.cpu().numpy()[agree], ref_cable[agree]) and np.array_equal(tape.cpu().numpy()[agree], ref_tape[agree])


def test_config5_1024_exact_vs_oracle_and_batch_invariance(torch_cuda, syn, oracle):
    """BASELINE config 5 shape (3-class 1024x1024): one frame against the oracle, and the size-independent
    property that a frame's result does not depend on its position in the batch (bitwise)."""
    torch = torch_cuda
    frames = syn.make_frames_u8(3, 1024, 1024, "smooth", 77)
    x = syn.frames_to_chw_f32(frames)
    model, sd = make_model(3, True, 2, "exact", syn, 3, (1024, 1024))
    xt = torch.from_numpy(x).cuda()
    mask, logits = model.segment(xt, return_logits=True)
    m1, l1 = model.segment(xt[2:3], return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(logits[2:3], l1) and torch.equal(mask[2:3], m1)
    ref = oracle.torch_forward(sd, x[:1])
    ref_mask, _, _ = oracle.masks_from_logits(ref)
    err, flips, unexplained = report(logits[:1].cpu().numpy(), mask[:1].cpu().numpy(), ref, ref_mask, oracle)
    print(f"1024x1024: max|dlogit|={err:.3e} flips={flips}/{ref_mask.size}")
    assert err < 3e-5 and unexplained == 0 and flips <= 8


def test_config4_7class_448x800_batch_properties(torch_cuda, syn, oracle):
    """BASELINE config 4 shape at batch 32 (exact): frames 0 and 31 of the batch against the oracle on the host,
    batch-row invariance and u8-vs-f32 input agreement."""
    torch = torch_cuda
    frames = syn.make_frames_u8(32, 448, 800, "smooth", 5)
    model, sd = make_model(7, False, 0, "exact", syn, 32, (448, 800))
    fu8 = torch.from_numpy(frames).cuda()
    mask, logits = model.segment(fu8, return_logits=True)
    torch.cuda.synchronize()
    ref = oracle.torch_forward(sd, syn.frames_to_chw_f32(frames[[0, 31]]))
    ref_mask, _, _ = oracle.masks_from_logits(ref)
    err, flips, unexplained = report(logits[[0, 31]].cpu().numpy(), mask[[0, 31]].cpu().numpy(), ref, ref_mask, oracle)
    print(f"config 4, B=32, frames 0 and 31 vs oracle: max|dlogit|={err:.3e} flips={flips}/{ref_mask.size}")
    assert err < 3e-5 and err < LOGIT_TOL and unexplained == 0 and flips <= 8
    m5 = model.segment(fu8[4:6])            # (two frames: like 32, too many tiles for a split-K plan -- equal plans, equal bits)
    mf = model.segment(torch.from_numpy(syn.frames_to_chw_f32(frames[30:32])).cuda())
    torch.cuda.synchronize()
    assert torch.equal(mask[4:6], m5) and torch.equal(mask[30:32], mf)
    hist = torch.bincount(mask.flatten().long(), minlength=7)
    assert int((hist > 0).sum()) >= 3 and int(hist.sum()) == 32 * 448 * 800


def test_fast_mode_error_is_bounded_and_reported(torch_cuda, syn, oracle):
    """fast (plain fp16) does not pass the 1e-3 gate; it must stay within its own documented band."""
    torch = torch_cuda
    frames = syn.make_frames_u8(2, 128, 160, "smooth", 9)
    x = syn.frames_to_chw_f32(frames)
    model, sd = make_model(3, True, 2, "fast", syn, 2, (128, 160))
    ref = oracle.torch_forward(sd, x)
    logits = model(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    err = float(np.abs(logits.cpu().numpy() - ref).max())
    print(f"fast 128x160: max|dlogit|={err:.3e}")
    assert 1e-5 < err < 3e-2


@pytest.mark.parametrize("tag", ["s_c3_64x64", "s_c3_128x96"])
def test_probabilities_and_class_rules(tag, torch_cuda, syn, oracle):
    """fused softmax + thresholded / strict / exclusive rules against the masks the
    reference's own functions produced.  A pixel may differ only if one of its probabilities sits within
    1e-5 of a decision boundary (the fp32 logits differ by ~1e-5 from the CPU's)."""
    from test_oracle_golden import RULE_CASES
    torch = torch_cuda
    g = load_golden(tag)
    B, H, W = int(g["B"]), int(g["H"]), int(g["W"])
    frames = syn.make_frames_u8(B, H, W, str(g["kind"]), int(g["fseed"]))
    model, _ = make_model(3, True, int(g["wseed"]), "exact", syn, B, (H, W))
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    probs = model.predict_proba(x)
    torch.cuda.synchronize()
    ref_p = np.transpose(g["probs_hwc"], (0, 3, 1, 2))
    perr = float(np.abs(probs.cpu().numpy() - ref_p).max())
    print(f"{tag}: max|dprob|={perr:.3e}")
    assert perr < 1e-5
    p0, p1, p2 = ref_p[:, 0], ref_p[:, 1], ref_p[:, 2]
    for key, rule, params in RULE_CASES:
        cable, tape = model.segment_thresholded(x, rule=rule, **params)
        torch.cuda.synchronize()
        cable, tape = cable.cpu().numpy(), tape.cpu().numpy()
        diff = (cable != g[f"rule_{key}_cable"]) | (tape != g[f"rule_{key}_tape"])
        # distance of each pixel to the nearest decision boundary of the rules
        tc, tt, bgm = params["t_cable"], params["t_tape"], params["bg_margin"]
        ctm = params.get("ct_margin", 0.0)
        d = np.minimum.reduce([np.abs(p1 - tc), np.abs(p2 - tt), np.abs(p1 - p0 - bgm), np.abs(p2 - p0 - bgm),
                               np.abs(p0 - bgm), np.abs(p1 - p2 - ctm), np.abs(p2 - p1 - ctm), np.abs(p1 - p2),
                               np.abs(p1 - p0), np.abs(p2 - p0)])
        print(f"  {key}: differing pixels {int(diff.sum())}")
        assert not (diff & (d > 1e-5)).any(), key
        assert int(diff.sum()) <= 3
        assert not (cable & tape).any()
    with pytest.raises(ValueError):
        model.segment_thresholded(x, rule="nope")


def test_mask_statistics_on_device(torch_cuda, syn, oracle):
    """class counts and per-row widths of the device mask equal the oracle's (and the
    reference function's golden widths) exactly — integer work, bit-exact."""
    torch = torch_cuda
    g = load_golden("s_c3_128x96")
    B, H, W = int(g["B"]), int(g["H"]), int(g["W"])
    frames = syn.make_frames_u8(B, H, W, str(g["kind"]), int(g["fseed"]))
    model, _ = make_model(3, True, int(g["wseed"]), "exact", syn, B, (H, W))
    mask = model.segment(torch.from_numpy(frames).cuda())
    counts, widths = model.mask_stats(mask)
    torch.cuda.synchronize()
    assert np.array_equal(mask.cpu().numpy(), g["mask"])
    ref_counts, ref_widths = oracle.mask_stats_np(g["mask"], 3)
    assert np.array_equal(counts.cpu().numpy(), ref_counts)
    assert np.array_equal(widths.cpu().numpy(), ref_widths)
    assert np.array_equal(widths.cpu().numpy()[:, 1], g["rowwidth_cable"])
    # ragged: random masks with empty rows, classes beyond num_classes ignored, W not a multiple of 256
    rng = np.random.default_rng(0)
    m = rng.integers(0, 5, (3, 37, 300), dtype=np.uint8)
    m[1, 5] = 0; m[2, :, :7] = 2
    c2, w2 = model.mask_stats(torch.from_numpy(m).cuda())
    rc, rw = oracle.mask_stats_np(np.where(m < 3, m, 255).astype(np.uint8), 3)
    rc = np.stack([[(m[b] == c).sum() for c in range(3)] for b in range(3)])
    assert np.array_equal(c2.cpu().numpy(), rc) and np.array_equal(w2.cpu().numpy(), rw)


@pytest.mark.parametrize("tag", ["su_c7_32x48", "su_c3_64x40", "su_c7_256x256"])
def test_simple_unet_matches_golden(tag, torch_cuda, syn, oracle):
    """SimpleUNet (conv3x3 + ReLU, pool, ConvTranspose2d k2 s2, cat([up, skip]), 1x1 head)
    against the reference class's outputs; 7-class 256x256 is the shape infer_video_simple.py:88 runs."""
    torch = torch_cuda
    from unet_amd.nested_unet import SimpleUNet
    g = load_golden(tag)
    B, H, W, C = int(g["B"]), int(g["H"]), int(g["W"]), int(g["num_classes"])
    frames = syn.make_frames_u8(B, H, W, str(g["kind"]), int(g["fseed"]))
    sd = syn.make_simple_state_dict(C, 3, int(g["wseed"]))
    model = SimpleUNet(num_classes=C, num_channels=3, max_batch=B, max_hw=(H, W)).to("cuda:0")
    model.load_state_dict(sd, strict=True)
    model.eval()
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    logits = model(x)
    probs = model.predict_proba(x)
    mask = model.segment(torch.from_numpy(frames).cuda())
    torch.cuda.synchronize()
    lg, pr, mk = logits.cpu().numpy(), probs.cpu().numpy(), mask.cpu().numpy()
    if "logits" in g.files:
        err = float(np.abs(lg - g["logits"]).max()); perr = float(np.abs(pr - g["probs"]).max())
        margin = oracle.top2_margin(g["logits"])
        assert not ((mk != g["mask"]) & (margin > 1e-4)).any()
        for k in [f for f in g.files if f.startswith("t_")]:
            got = model.debug_activation(k[2:], B, H, W)
            np.testing.assert_allclose(got, g[k], rtol=0, atol=3e-5, err_msg=k)
    else:
        err = float(np.abs(lg[:, :, ::4, ::4] - g["logits_sub4"]).max()); perr = float(np.abs(pr[:, :, ::4, ::4] - g["probs_sub4"]).max())
        ties = {tuple(t) for t in g["tie_idx"].tolist()}
        assert all(tuple(d) in ties for d in np.argwhere(mk != g["mask"]).tolist())
    print(f"{tag}: max|dlogit|={err:.3e} max|dprob|={perr:.3e} mask diffs={int((mk != g['mask']).sum())}")
    assert err < 5e-5 and perr < 1e-5
    with pytest.raises(RuntimeError, match="multiples of 8"):
        model(torch.zeros(1, 3, 36, 32, device="cuda"))


def test_simple_unet_fast_and_batch_invariance(torch_cuda, syn, oracle):
    torch = torch_cuda
    from unet_amd.nested_unet import SimpleUNet
    sd = syn.make_simple_state_dict(7, 3, 0)
    frames = syn.make_frames_u8(3, 64, 96, "smooth", 41)
    x = syn.frames_to_chw_f32(frames)
    ref = oracle.simple_unet_torch_forward(sd, x)
    xt = torch.from_numpy(x).cuda()
    for prec, tol in (("exact", SIMPLE_EXACT_TOL), ("fast", SIMPLE_FAST_TOL)):
        m = SimpleUNet(7, precision=prec, max_batch=3, max_hw=(64, 96)).to("cuda:0")
        m.load_state_dict(sd)
        a = m(xt); b = m(xt[1:2])
        torch.cuda.synchronize()
        assert torch.equal(a[1:2], b)
        err = float(np.abs(a.cpu().numpy() - ref).max())
        print(f"simple {prec}: max|dlogit|={err:.3e}")
        assert err < tol


def test_engine_reuse_smaller_shapes_and_two_engines(torch_cuda, syn, oracle):
    """One engine sized for 128x160 serves smaller shapes and batches without rebuilding; two engines
    (different class counts / precisions) coexist on the device."""
    torch = torch_cuda
    big, sd = make_model(3, True, 2, "exact", syn, 4, (128, 160))
    other, sd7 = make_model(7, False, 0, "fast", syn, 2, (64, 64))
    ws = None
    for (B, H, W) in ((4, 128, 160), (1, 48, 64), (3, 16, 160), (2, 128, 32)):
        frames = syn.make_frames_u8(B, H, W, "uniform", H + W)
        x = syn.frames_to_chw_f32(frames)
        ref = oracle.torch_forward(sd, x)
        got = big(torch.from_numpy(x).cuda())
        m7 = other.segment(torch.zeros(2, 3, 64, 64, device="cuda"))
        torch.cuda.synchronize()
        assert float(np.abs(got.cpu().numpy() - ref).max()) < 2e-5
        assert m7.shape == (2, 64, 64)
        ws = ws or big.workspace_bytes()                    # engine is created lazily at the first forward
    assert big.workspace_bytes() == ws                      # never re-created
    with pytest.raises(RuntimeError, match="too large"):
        from unet_amd.nested_unet import NestedUNet
        huge = NestedUNet(3, max_batch=1, max_hw=(8192, 8192)).to("cuda:0")
        huge.load_state_dict(sd)
        huge(torch.zeros(1, 3, 16, 16, device="cuda"))


# ---- the cv2.resize steps either side of the model (parity unpinned: cv2 absent; the
# oracle restates OpenCV's published fixed-point INTER_LINEAR / INTER_NEAREST, the device must match it bit for bit)
@pytest.mark.parametrize("shape,dsize", [((2, 1080, 1920, 3), (512, 512)), ((1, 480, 640, 3), (800, 448)),
                                         ((3, 37, 53, 1), (16, 16)), ((1, 64, 48, 3), (48, 64)),
                                         ((2, 5, 7, 3), (31, 13)), ((1, 720, 1280, 4), (510, 254))])
def test_resize_linear_matches_cv2_restatement(shape, dsize, torch_cuda, syn, oracle):
    torch = torch_cuda
    rng = np.random.default_rng(shape[1] * 7 + shape[2])
    frames = rng.integers(0, 256, shape, dtype=np.uint8)
    model, _ = make_model(3, True, 2, "exact", syn, 1, (16, 16))
    got = model.resize_frames(torch.from_numpy(frames).cuda(), (dsize[1], dsize[0]))
    torch.cuda.synchronize()
    assert got.shape == (shape[0], dsize[1], dsize[0], shape[3])
    for b in range(shape[0]):
        ref = oracle.cv2_resize_linear_u8_np(frames[b], dsize)
        assert np.array_equal(got[b].cpu().numpy(), ref.reshape(dsize[1], dsize[0], shape[3])), f"frame {b}"


@pytest.mark.parametrize("src_hw,frame_wh,roi", [((512, 512), (1920, 1080), (525, 0, 1012, 1080)),
                                                  ((512, 512), (1080, 1920), None),
                                                  ((64, 96), (333, 127), (10, 5, 400, 90)),
                                                  ((48, 80), (80, 48), (0, 0, 0, 0)),
                                                  ((128, 128), (50, 30), (7, 3, 8, 4))])
def test_resize_nearest_roi_matches_restatement(src_hw, frame_wh, roi, torch_cuda, syn, oracle):
    torch = torch_cuda
    rng = np.random.default_rng(src_hw[0] + frame_wh[0])
    pred = rng.integers(0, 3, (2,) + src_hw, dtype=np.uint8)
    model, _ = make_model(3, True, 2, "exact", syn, 1, (16, 16))
    d = torch.from_numpy(pred).cuda()
    for cls in (-1, 1, 2):
        got = model.resize_masks(d, frame_wh, match_class=cls, roi=roi).cpu().numpy()
        for b in range(2):
            m = pred[b] if cls < 0 else (pred[b] == cls).astype(np.uint8)
            ref = oracle.cv2_resize_nearest_np(m, frame_wh)
            if roi is not None:
                ref = oracle.clip_to_roi_np(ref, roi)
            assert np.array_equal(got[b], ref), (cls, b)
    with pytest.raises(RuntimeError, match="negative ROI"):
        model.resize_masks(d, frame_wh, roi=(-1, 0, 5, 5))


def test_process_frames_whole_loop_on_device(torch_cuda, syn, oracle):
    """Raw BGR frames -> resize -> model -> argmax -> class masks at frame size inside the ROI, against the same
    chain on the CPU (oracle preprocess_image_np -> torch_segment -> postprocess_masks_np)."""
    torch = torch_cuda
    from unet_amd.frame_loop import process_frames, map_roi_to_original
    fh, fw, th, tw = 270, 480, 96, 128
    frames = syn.make_frames_u8(3, fh, fw, "smooth", 40)
    model, sd = make_model(3, True, 2, "exact", syn, 3, (th, tw))
    pred, cable, tape = process_frames(model, frames, target_size=(tw, th), roi="fixed")
    torch.cuda.synchronize()
    roi = map_roi_to_original((fw, fh), (tw, th))
    assert cable.shape == (3, fh, fw) and tape.shape == (3, fh, fw)
    for b in range(3):
        x = oracle.preprocess_image_np(frames[b], (tw, th))[None]
        ref_logits = oracle.torch_forward(sd, x)
        ref_pred = oracle.masks_from_logits(ref_logits)[0][0]          # [H,W]
        got_pred = pred[b].cpu().numpy()
        flips = got_pred != ref_pred
        assert not (flips & (oracle.top2_margin(ref_logits)[0] > 1e-4)).any()
        # the glue after the model is integer work: exact given the device's own pred
        rc, rt = oracle.postprocess_masks_np(got_pred, (fw, fh), roi)
        assert np.array_equal(cable[b].cpu().numpy(), rc) and np.array_equal(tape[b].cpu().numpy(), rt)
        if not flips.any():
            rc2, rt2 = oracle.postprocess_masks_np(ref_pred, (fw, fh), roi)
            assert np.array_equal(cable[b].cpu().numpy(), rc2) and np.array_equal(tape[b].cpu().numpy(), rt2)


def test_determinism_side_stream_and_threads(torch_cuda, syn):
    """Same input -> bitwise the same logits: run to run, on a non-default stream, and from two host threads
    driving two independent engines at once (include/unetpp.h: an engine is not thread-safe, independent engines are)."""
    import threading
    torch = torch_cuda
    B, H, W = 3, 96, 160
    frames = syn.make_frames_u8(B, H, W, "smooth", 9)
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    m1, _ = make_model(3, True, 2, "exact", syn, B, (H, W))
    m2, _ = make_model(3, True, 2, "exact", syn, B, (H, W))
    a = m1(x)
    b = m1(x)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = m1(x)
        mask_side = m1.segment(x)
    side.synchronize()
    assert torch.equal(a, c) and torch.equal(mask_side, a.argmax(1).to(torch.uint8))
    results = {}

    def worker(name, model):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            outs = [model(x) for _ in range(5)]
        s.synchronize()
        results[name] = outs
    ts = [threading.Thread(target=worker, args=(n, m)) for n, m in (("m1", m1), ("m2", m2))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for outs in results.values():
        assert len(outs) == 5 and all(torch.equal(o, a) for o in outs)


def test_lock_step_small_grid_tiles_are_bitwise_the_same(torch_cuda, syn, monkeypatch):
    """The lock-step kernel (every conv of fast mode; SimpleUNet's two-source decoder convs in exact mode) runs small
    batches' pool-free layers with 8-row tiles (twice the workgroups) and large ones with 16-row tiles; a frame's logits
    must not depend on which tile height computed it.  (UNETPP_KSPLIT=1: the wave-specialised layers of exact mode keep one
    launch plan for every batch size, so the tile height is the only thing that changes.)"""
    torch = torch_cuda
    from unet_amd.nested_unet import SimpleUNet
    monkeypatch.setenv("UNETPP_KSPLIT", "1")
    B, H, W = 16, 256, 256
    frames = syn.make_frames_u8(B, H, W, "smooth", 31)
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    simple = SimpleUNet(num_classes=7, max_batch=B, max_hw=(H, W)).to("cuda:0")
    simple.load_state_dict(syn.make_simple_state_dict(7, 3, 2), strict=True)
    fast, _ = make_model(3, True, 2, "fast", syn, B, (H, W))
    # a lock-step layer whose tile count crosses the CU count between 1 and 16 frames: exact SimpleUNet dec3.0 (256
    # channels at 64x64: 32 -> 512 tiles); fast conv1_3.conv2 (64 channels at 128x128: 32 -> 512)
    for prec, m, layer in (("exact", simple.eval(), "dec3.0"), ("fast", fast, "conv1_3.conv2")):
        m(x[:1])                                   # creates the engine
        m.profile(True)
        one = m(x[:1])
        torch.cuda.synchronize()
        names_1 = [r[0] for r in m.profile_read()]
        m.profile(True)
        full = m(x)
        torch.cuda.synchronize()
        names_b = [r[0] for r in m.profile_read()]
        m.profile(False)
        pick = lambda names, layer: next(n for n in names if n.startswith(layer + "|"))
        rows = lambda n: int(n.split("<")[1].split(",")[3])          # the MW template argument
        assert "conv3x3_bias_relu_kernel<" in pick(names_1, layer), prec
        assert rows(pick(names_1, layer)) == 1 and rows(pick(names_b, layer)) == 2
        assert torch.equal(one, full[:1]), prec


def test_random_shapes_against_oracle(torch_cuda, syn, oracle):
    """Seeded sweep over (classes, batch, H, W, weight seed): every case against the CPU oracle."""
    torch = torch_cuda
    rng = np.random.default_rng(20261004)
    for _ in range(12):
        C = int(rng.integers(1, 9)); B = int(rng.integers(1, 4))
        H = 16 * int(rng.integers(1, 11)); W = 16 * int(rng.integers(1, 11))
        wseed = int(rng.integers(0, 50))
        frames = syn.make_frames_u8(B, H, W, "smooth" if rng.integers(0, 2) else "uniform", int(rng.integers(0, 1000)))
        x = syn.frames_to_chw_f32(frames)
        model, sd = make_model(C, C == 3, wseed, "exact", syn, B, (H, W))
        ref = oracle.torch_forward(sd, x)
        mask, logits = model.segment(torch.from_numpy(x).cuda(), return_logits=True)
        torch.cuda.synchronize()
        err, flips, unexplained = report(logits.cpu().numpy(), mask.cpu().numpy(), ref, oracle.masks_from_logits(ref)[0], oracle)
        scale = max(1.0, float(np.abs(ref).max()))
        assert err < 2e-5 * scale and unexplained == 0, (C, B, H, W, wseed, err, flips)


def test_simple_unet_random_shapes_against_oracle(torch_cuda, syn, oracle):
    """The same sweep for SimpleUNet (H, W multiples of 8; transposed-conv upsampling)."""
    torch = torch_cuda
    from unet_amd.nested_unet import SimpleUNet
    rng = np.random.default_rng(41001)
    for _ in range(8):
        C = int(rng.integers(1, 9)); B = int(rng.integers(1, 4))
        H = 8 * int(rng.integers(1, 17)); W = 8 * int(rng.integers(1, 17))
        sd = syn.make_simple_state_dict(C, 3, int(rng.integers(0, 50)))
        x = syn.frames_to_chw_f32(syn.make_frames_u8(B, H, W, "smooth", int(rng.integers(0, 1000))))
        m = SimpleUNet(num_classes=C, num_channels=3, max_batch=B, max_hw=(H, W)).to("cuda:0")
        m.load_state_dict(sd, strict=True)
        ref = oracle.simple_unet_torch_forward(sd, x)
        mask, logits = m.segment(torch.from_numpy(x).cuda(), return_logits=True)
        torch.cuda.synchronize()
        err, flips, unexplained = report(logits.cpu().numpy(), mask.cpu().numpy(), ref, oracle.masks_from_logits(ref)[0], oracle)
        assert err < 5e-5 * max(1.0, float(np.abs(ref).max())) and unexplained == 0, (C, B, H, W, err, flips)


def _b16_inputs(syn, g):
    kinds = [str(k) for k in g["kinds"]]
    B, H, W = int(g["B"]), int(g["H"]), int(g["W"])
    frames = np.stack([syn.make_frame_u8(H, W, i, kinds[i % len(kinds)], int(g["fseed"])) for i in range(B)])
    assert hashlib.sha256(frames.tobytes()).hexdigest() == str(g["frames_sha"])
    return frames


def test_config2_batch16_against_reference_fixture(torch_cuda, syn, oracle):
    """BASELINE config 2 at its stated batch: 16 frames (smooth and uniform) of 3-class 512x512 through ONE forward,
    against masks / near-tie list / 8x-subsampled logits the reference itself produced (oracle/make_golden.py), and
    per-layer against the reference's x0_0 ... x0_4 of frames 0-1 sampled at seeded random positions — at this size
    every node spans many tiles, so a tiling regression is located, not just detected."""
    torch = torch_cuda
    g = load_golden("b_c3_512x512_b16")
    frames = _b16_inputs(syn, g)
    model, _ = make_model(3, True, int(g["wseed"]), "exact", syn, 16, (512, 512))
    xt = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    mask, logits = model.segment(xt, return_logits=True)
    torch.cuda.synchronize()
    lg = logits.cpu().numpy(); mk = mask.cpu().numpy()
    sub = float(np.abs(lg[:, :, ::8, ::8] - g["logits_sub8"]).max())
    diff = np.argwhere(mk != g["mask"])
    ties = {tuple(t) for t in g["tie_idx"].tolist()}
    print(f"config 2, B=16: sub8 max|dlogit|={sub:.3e}, {len(diff)} of {mk.size} mask pixels differ "
          f"({len(diff) / mk.size:.2e} per pixel), near-ties listed: {len(ties)}")
    assert sub < 2e-5 and sub < LOGIT_TOL
    assert all(tuple(d) in ties for d in diff.tolist())          # only listed near-tie pixels (margin < 1e-3) may differ
    assert len(diff) <= 24                                       # ~1.5 per frame at round 1 (7 of 16 frames' pixels)
    # the device mask is the argmax of the device's own logits (same rule as np.argmax(softmax)), except where the
    # two best probabilities coincide after exp() rounding
    own_mask, _, _ = oracle.masks_from_logits(lg)
    p = oracle.softmax_np(lg, axis=1)
    ps = np.sort(p, axis=1)
    assert np.array_equal(mk[ps[:, -1] != ps[:, -2]], own_mask[ps[:, -1] != ps[:, -2]])
    # per-layer, frames 0-1
    model.debug_keep_intermediates(True)
    model(xt[:2])
    torch.cuda.synchronize()
    for name in NODES:
        got = model.debug_activation(name, 2, 512, 512)
        ys, xs = g["p_" + name][:, 0], g["p_" + name][:, 1]
        np.testing.assert_allclose(got[:, :, ys, xs], g["t_" + name], rtol=0, atol=3e-5, err_msg=name)
    assert model.status() == 0


def test_config5_1024_batch8_against_reference_fixture(torch_cuda, syn, oracle):
    """BASELINE config 5 at its stated batch of 8: frame 0 against the reference's own output (fixture), every other
    frame through batch-row invariance (its result alone == its row of the batch, bitwise)."""
    torch = torch_cuda
    g = load_golden("b_c3_1024x1024")
    frames = syn.make_frames_u8(8, 1024, 1024, "smooth", int(g["fseed"]))
    assert hashlib.sha256(frames[:1].tobytes()).hexdigest() == str(g["frames_sha"])
    model, _ = make_model(3, True, int(g["wseed"]), "exact", syn, 8, (1024, 1024))
    xu8 = torch.from_numpy(frames).cuda()
    mask, logits = model.segment(xu8, return_logits=True)
    torch.cuda.synchronize()
    sub = float(np.abs(logits[:1, :, ::8, ::8].cpu().numpy() - g["logits_sub8"]).max())
    diff = np.argwhere(mask[:1].cpu().numpy() != g["mask"])
    ties = {tuple(t) for t in g["tie_idx"].tolist()}
    print(f"config 5, B=8: frame 0 sub8 max|dlogit|={sub:.3e}, {len(diff)} of {1024 * 1024} mask pixels differ")
    assert sub < 3e-5 and all(tuple(d) in ties for d in diff.tolist()) and len(diff) <= 8
    for i in range(1, 8):
        mi, li = model.segment(xu8[i:i + 1], return_logits=True)
        assert torch.equal(li, logits[i:i + 1]) and torch.equal(mi, mask[i:i + 1])
    assert model.status() == 0


@pytest.mark.parametrize("env", [{"UNETPP_KSPLIT": "1"}, {"UNETPP_TAPMM": "2"}, {"UNETPP_KSPLIT": "2"}, {"UNETPP_TAPMM": "none"},
                                 {"UNETPP_TAPMM": "3"}, {"UNETPP_TAPMM": "none", "UNETPP_KSPLIT": "1"}])
def test_alternative_kernel_paths_agree(env, torch_cuda, syn, oracle, monkeypatch):
    """The two switches read when an engine is created pick between live plans of the exact-mode path: UNETPP_TAPMM which
    decoder levels take the low-resolution GEMM (the others interpolate their up channels in the wave-specialised loader),
    UNETPP_KSPLIT the split-K of small launches (this 96x160 batch of 2 splits levels 3-4 by default; "1" = no split, "2" =
    two-way splits at most).  Each plan must pass the same parity bar as the default path and agree with it to rounding
    (the summation order differs, the arithmetic does not)."""
    torch = torch_cuda
    frames = syn.make_frames_u8(2, 96, 160, "smooth", 41)
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    base, sd = make_model(3, True, 2, "exact", syn, 2, (96, 160))
    ref = oracle.torch_forward(sd, syn.frames_to_chw_f32(frames))
    ref_mask, _, _ = oracle.masks_from_logits(ref)
    m0, l0 = base.segment(x, return_logits=True)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    alt, _ = make_model(3, True, 2, "exact", syn, 2, (96, 160))
    m1, l1 = alt.segment(x, return_logits=True)
    torch.cuda.synchronize()
    for name, lg, mk in (("default", l0, m0), (str(env), l1, m1)):
        err, flips, unexplained = report(lg.cpu().numpy(), mk.cpu().numpy(), ref, ref_mask, oracle)
        print(f"{name}: max|dlogit|={err:.3e} flips={flips}")
        assert err < 2e-5 and unexplained == 0
    assert float((l0 - l1).abs().max()) < 2e-5
    assert alt.status() == 0 and base.status() == 0
