"""The probability-map rules on the device (unetpp_prob_levels_f32, unetpp_prob_threshold_hist_f32,
unetpp_components_prob_sum_f32, unetpp_components_filter_mean and the functions of unet_amd/probmap.py) against the NumPy
forms and the fixtures made from the reference's own functions.  Comparisons of float32 values and integer sums:
equality everywhere, no tolerance."""
import ctypes

import numpy as np
import pytest

from test_probmap_host import CASES, G, SETS, TAGS, results_table, scene, scene_set, stored
from unet_amd import components as cc
from unet_amd import probmap as pm
from unet_amd import tiling as tl

pytestmark = pytest.mark.gpu

NAN = np.float32(np.nan)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def model(torch_cuda):
    from unet_amd.nested_unet import NestedUNet
    return NestedUNet(3, max_batch=1, max_hw=(16, 16)).to("cuda:0")      # no weights: only the loop test needs any


@pytest.fixture(scope="module")
def span():
    n = pm.layout()
    assert n >= 256 and n % 16 == 0
    return n


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def embedded(torch, a, offset):
    """A CUDA view of a's shape at ELEMENT `offset` of a larger buffer whose other elements are 2.0 and NaN in turn (uint8,
    int32: 255): a value read outside the view lands in the top bin, or in bin 0 where none belongs."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if a.dtype == np.float32:
        buf = torch.full((a.size + offset + 64,), 2.0, dtype=torch.float32, device="cuda")
        buf[1::2] = float("nan")
    else:
        buf = torch.full((a.size + offset + 64,), 255, dtype=t.dtype, device="cuda")
    view = buf[offset:offset + a.size].view(*a.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + offset * a.itemsize
    return view


def special_values(thr):
    out = [0.0, 1.0, -0.0, np.nan, 2.0, -1.0, np.inf, -np.inf, 1e-45, 2.0 ** -32, 2.0 ** -33, 1e-10]
    for t in np.asarray(thr, np.float32):
        out += [t, np.nextafter(t, np.float32(-1)), np.nextafter(t, np.float32(2))]
    return np.array(out, np.float32)


def random_plane(shape, thr, seed, strides=1):
    """float32 shape + (strides,): runs of plateaus and noise, with every special value in every channel when it fits."""
    r = np.random.default_rng(seed)
    full = tuple(shape) + (strides,)
    p = r.random(full).astype(np.float32)
    plateau = r.random(full) < 0.5
    p[plateau] = np.float32(0.8)
    sp = special_values(thr)
    flat = p.reshape(-1, strides)
    n = min(len(sp), len(flat))
    where = r.choice(len(flat), n, replace=False)
    for c in range(strides):
        flat[where, c] = np.roll(sp, c)[:n]
    return p


def random_target(shape, seed):
    r = np.random.default_rng(seed + 1000)
    t = r.integers(0, 4, shape).astype(np.uint8)
    t[r.random(shape) < 0.5] = 0
    return t


THR3 = np.array([0.25, 0.5, 0.8], np.float32)


def check_plane(torch, model, p, target, thr, offsets=(0,), **kw):
    """Levels and histogram of every channel of p [B,H,W,S] (S = 1 also as [B,H,W]) at every offset, against NumPy."""
    s = p.shape[-1]
    for off in offsets:
        pd = embedded(torch, p, off)
        td = embedded(torch, target, off)
        for c in range(s):
            views = [(pd, c)] + ([(pd[..., 0], None)] if s == 1 else [])
            for view, ch in views:
                want = pm.levels_np(p, thr[0], thr[-1], channel=c)
                got = pm.threshold_levels(model, view, thr[0], thr[-1], channel=ch)
                assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (p.shape, off, c)
                want_h, want_o = pm.threshold_hist_np(p, target, thr, channel=c, return_outside=True, **kw)
                got_h, got_o = pm.threshold_histogram(model, view, td, thr, channel=ch, return_outside=True, **kw)
                assert got_h.dtype == torch.int64 and got_h.is_cuda and tuple(got_h.shape) == want_h.shape
                assert np.array_equal(got_h.cpu().numpy(), want_h) and np.array_equal(got_o.cpu().numpy(), want_o), (p.shape, off, c)
                assert np.array_equal(want_h.sum((1, 2)) + want_o, np.full(p.shape[0], p.shape[1] * p.shape[2]))


# ---- 1. levels and histogram: shapes, strides, alignments, values ---------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 1, 1), (3, 5, 7), (2, 1, 16), (2, 1, 17), (5, 3, 21)])
def test_smallest_and_misaligned_shapes(torch_cuda, model, shape):
    target = random_target(shape, 1)
    for s in (1, 2, 3, 7):
        check_plane(torch_cuda, model, random_plane(shape, THR3, 10 + s, s), target, THR3, offsets=(0, 1, 3, 6))


@pytest.mark.parametrize("extra", [-1, 0, 1])
def test_one_workgroup_span_and_a_pixel_more(torch_cuda, model, span, extra):
    shape = (2, 1, span + extra)
    target = random_target(shape, 2)
    for s in (1, 2, 3):
        check_plane(torch_cuda, model, random_plane(shape, THR3, 20 + s, s), target, THR3, offsets=(0, 1, 2))


def test_special_values_land_in_their_bins(torch_cuda, model):
    """Values at each threshold, one ulp either side, 0, 1, -0.0, NaN, infinities and values outside [0,1], one per pixel."""
    thr = pm.check_thresholds(pm.scan_values())
    sp = special_values(thr)
    p = np.resize(sp, (2, 1, len(sp) + 5)).astype(np.float32)[..., None]
    target = (np.arange(p[..., 0].size).reshape(p.shape[:3]) % 2).astype(np.uint8)
    check_plane(torch_cuda, model, p, target, thr, offsets=(0, 1))
    k = pm.threshold_hist_np(p[..., 0][:1, :, :len(sp)], np.ones((1, 1, len(sp)), np.uint8), thr)[0, 1]
    assert k[0] >= 8 and k[-1] >= 3                            # NaN, zeros, negatives, tiny values / 1, 2, inf


@pytest.mark.parametrize("T", [1, 25, 49, 256])
def test_threshold_counts(torch_cuda, model, T):
    thr = np.linspace(0.02, 0.99, T).astype(np.float32) if T > 1 else np.array([0.5], np.float32)
    shape = (2, 37, 53)
    check_plane(torch_cuda, model, random_plane(shape, thr, 30 + T, 2), random_target(shape, 3), thr)
    check_plane(torch_cuda, model, random_plane(shape, thr, 31 + T, 1), random_target(shape, 4), thr, target_class=2)


def test_one_bin_holds_a_whole_frame(torch_cuda, model):
    """The contended case: every pixel in one bin, more of them than 16 bits count."""
    shape = (2, 300, 301)
    p = np.full(shape + (1,), 0.95, np.float32)
    p[1] = NAN
    target = np.ones(shape, np.uint8)
    thr = pm.check_thresholds(pm.scan_values())
    check_plane(torch_cuda, model, p, target, thr)
    hist = pm.threshold_hist_np(p[..., 0], target, thr)
    assert hist[0, 1].max() == 300 * 301 == hist[1, 1, 0] and np.count_nonzero(hist) == 2


def test_ignore_value_and_target_class(torch_cuda, model):
    shape = (3, 33, 57)
    p = random_plane(shape, THR3, 40, 2)
    target = random_target(shape, 5)
    target[:, :3] = 255
    check_plane(torch_cuda, model, p, target, THR3, ignore_value=255)
    check_plane(torch_cuda, model, p, target, THR3, ignore_value=0, target_class=3)
    _, outside = pm.threshold_hist_np(p, target, THR3, channel=0, ignore_value=255, return_outside=True)
    assert outside.tolist() == [3 * 57] * 3


def test_running_total_over_two_calls(torch_cuda, model):
    torch = torch_cuda
    thr = pm.check_thresholds(pm.scan_values((0.5, 0.99, 0.02)))
    want = np.zeros((2 * (len(thr) + 1) + 1,), np.int64)
    total = torch.zeros_like(dev(torch, want))
    for seed, shape in ((50, (2, 40, 64)), (51, (1, 33, 57))):
        p, target = random_plane(shape, thr, seed, 1)[..., 0], random_target(shape, seed)
        target[:, 0] = 7
        pm.threshold_hist_np(p, target, thr, ignore_value=7, total=want)
        pm.threshold_histogram(model, dev(torch, p), dev(torch, target), thr, ignore_value=7, total=total)
    assert want[-1] == 2 * 64 + 57 and np.array_equal(total.cpu().numpy(), want)
    with pytest.raises(ValueError, match="total"):
        pm.threshold_histogram(model, dev(torch, p), dev(torch, target), thr, total=total[:-1])


# ---- 2. sums and the mean rule ------------------------------------------------------------------------------------------------------
def components_of(torch, model, mask, k=64):
    labels, num, stats, _ = model.components(dev(torch, mask), -1, 8, k)
    return labels, num, stats


def test_exact_tie_is_kept_and_one_ulp_drops_it(torch_cuda, model, span):
    """0.5 and 0.75 in equal numbers against 0.625: the tie stays, one pixel an ulp lower drops the component.  The large
    block spans several workgroups, the small one sits inside one wave's pixels; kernel_size 1 leaves the mask alone."""
    torch = torch_cuda
    H, W = 96, 128
    assert H * W >= 3 * span
    mask = np.zeros((2, H, W), np.uint8)
    prob = np.full((2, H, W), 0.99, np.float32)
    mask[:, 4:84, 10:110] = 1
    prob[:, 4:84, 10:60], prob[:, 4:84, 60:110] = 0.5, 0.75
    mask[:, 90:94, 4:8] = 1
    prob[:, 90:94, 4:6], prob[:, 90:94, 6:8] = 0.75, 0.5
    prob[1, 40, 30] = np.nextafter(np.float32(0.5), np.float32(0))
    prob[1, 91, 5] = np.nextafter(np.float32(0.75), np.float32(0))
    want = pm.filter_mean_prob_np(mask, prob, 16, 0.625, kernel_size=1)
    assert np.array_equal(want[0], mask[0]) and not want[1].any()
    got = pm.filter_by_mean_prob(model, dev(torch, mask), dev(torch, prob), 16, 0.625, kernel_size=1)
    assert np.array_equal(got.cpu().numpy(), want)
    labels, num, stats = components_of(torch, model, mask)
    sums = pm.component_prob_sums(model, labels, num, dev(torch, prob), max_components=64).cpu().numpy().view(np.uint64)
    assert sums[0, 1] == 8000 * 5 * (1 << 29) and sums[0, 2] == 16 * 5 * (1 << 29) and sums[1, 1] == sums[0, 1] - 128
    assert np.array_equal(sums, pm.prob_sums_np(labels.cpu().numpy(), prob, 64))


def test_full_frame_of_ones_and_tiny_values(torch_cuda, model):
    torch = torch_cuda
    mask = np.ones((2, 64, 64), np.uint8)
    prob = np.ones((2, 64, 64), np.float32)
    tiny = np.float32([1e-45, 1e-40, 2.0 ** -33, 2.0 ** -32, 3 * 2.0 ** -32, 1e-9, -0.0, -1e-3, np.nan, 2.0, np.inf, 0.3])
    prob[1] = np.resize(tiny, (64, 64))
    labels, num, stats = components_of(torch, model, mask)
    sums = pm.component_prob_sums(model, labels, num, dev(torch, prob), max_components=64).cpu().numpy().view(np.uint64)
    assert sums[0, 1] == 4096 << 32 and not sums[:, 0].any() and not sums[:, 2:].any()
    assert np.array_equal(sums, pm.prob_sums_np(labels.cpu().numpy(), prob, 64)) and sums[1, 1] == pm.q32_np(prob[1]).sum()
    got = pm.filter_by_mean_prob(model, dev(torch, mask), dev(torch, prob), 50, 1.0, kernel_size=1).cpu().numpy()
    assert got[0].all() and not got[1].any()


@pytest.mark.parametrize("strides", [1, 2, 3])
def test_sums_on_scene_components_strides_and_offsets(torch_cuda, model, strides):
    torch = torch_cuda
    shape = (2, 45, 77)
    mask = np.stack([cc.make_scene_mask(45, 77, s, noise=0.05) for s in (0, 1)])
    p = random_plane(shape, THR3, 60 + strides, strides)
    labels, num, stats = components_of(torch, model, mask, 4096)
    lab = labels.cpu().numpy()
    assert num.max() > 20
    for off in (0, 1, 2):
        ld, pd = embedded(torch, lab, off), embedded(torch, p, off)
        for c in range(strides):
            for k in (4096, 8):                                # 8: most labels lie above the capacity and are left out
                got = pm.component_prob_sums(model, ld, num, pd, c, k).cpu().numpy().view(np.uint64)
                assert np.array_equal(got, pm.prob_sums_np(lab, p, k, channel=c)), (off, c, k)


def test_zero_components_and_too_many(torch_cuda, model):
    torch = torch_cuda
    prob = dev(torch, np.full((2, 20, 30), 0.95, np.float32))
    empty = torch.zeros((2, 20, 30), dtype=torch.uint8, device="cuda")
    assert not pm.filter_by_mean_prob(model, empty, prob, 1, 0.5).any()
    dots = np.zeros((2, 20, 30), np.uint8)
    dots[1, ::2, ::2] = 1                                      # 150 components in the second frame
    with pytest.raises(RuntimeError, match="max_components"):
        pm.filter_by_mean_prob(model, dev(torch, dots), prob, 1, 0.5, kernel_size=1, max_components=16)
    assert not pm.filter_by_mean_prob(model, dev(torch, dots), prob, 1, 0.5, kernel_size=1, max_components=16, check=False).any()
    assert np.array_equal(pm.filter_by_mean_prob(model, dev(torch, dots), prob, 1, 0.5, kernel_size=1, max_components=256).cpu().numpy(), dots)


def test_the_same_call_twice_gives_the_same_bytes(torch_cuda, model):
    torch = torch_cuda
    c = CASES[0]
    prob, target = scene(c)
    pd, td = dev(torch, np.stack([prob, prob[::-1]])), dev(torch, np.stack([target, target]))
    runs = []
    for _ in range(2):
        hyst, final = pm.postprocess_probmap(model, pd)
        labels, num, stats = components_of(torch, model, hyst.cpu().numpy(), 256)
        sums = pm.component_prob_sums(model, labels, num, pd, max_components=256)
        hist = pm.threshold_histogram(model, pd, td, pm.scan_values())
        runs.append(b"".join(x.cpu().numpy().tobytes() for x in (hyst, final, sums, hist)))
    assert runs[0] == runs[1]


# ---- 3. the compositions against the reference's stored results ------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_fixture_masks(torch_cuda, model, tag):
    torch = torch_cuda
    prob, _ = scene(CASES[TAGS.index(tag)])
    want_h, want_f = stored(tag, "hyst", prob.shape), stored(tag, "final", prob.shape)
    pd = dev(torch, prob[None])
    hyst = pm.hysteresis(model, pd)
    assert hyst.dtype == torch.uint8 and np.array_equal(hyst[0].cpu().numpy(), want_h)
    assert np.array_equal(pm.filter_by_mean_prob(model, dev(torch, want_h[None]), pd)[0].cpu().numpy(), want_f)
    two = dev(torch, np.stack([1 - prob, prob], -1)[None])                        # class 1 of [B,H,W,2], read in place
    got_h, got_f = pm.postprocess_probmap(model, two, channel=1, out_value=255)
    assert np.array_equal(got_h[0].cpu().numpy(), want_h * 255) and np.array_equal(got_f[0].cpu().numpy(), want_f * 255)


@pytest.mark.parametrize("name", [s["name"] for s in SETS])
def test_fixture_scan(torch_cuda, model, name):
    torch = torch_cuda
    s = next(x for x in SETS if x["name"] == name)
    probs, targets = scene_set(s)
    got = pm.scan_thresholds(model, [dev(torch, p) for p in probs], [dev(torch, t) for t in targets], s["thr_range"])
    assert [float(v) for v in got[:3]] == G[name + "_thr"].tolist()
    assert np.array_equal(results_table(got[3]), G[name + "_results"])


def test_process_frames_optimized(torch_cuda, syn):
    """The whole loop on a small frame with synthetic weights against tiling.predict_tiled_np composed with the NumPy forms,
    fed the device's own per-patch maps: the network is the engine's on both sides, everything after it must agree bit for
    bit.  The thresholds are quantiles of the map itself, so that every rule has something to decide."""
    torch = torch_cuda
    from unet_amd import frame_loop
    from unet_amd.nested_unet import NestedUNet
    m = NestedUNet(2, deep_supervision=False, precision="exact", max_batch=4, max_hw=(16, 16)).to("cuda:0")
    m.load_state_dict(syn.make_trained_like_state_dict(2, 3, False, 0), strict=True)
    m.eval()
    frame = np.ascontiguousarray(syn.make_frame_u8(48, 70, 3, "uniform", 11))
    seen = {}

    def model_fn(tiles):
        maps = np.concatenate([m.predict_proba(dev(torch, tiles[k:k + 4])).cpu().numpy() for k in range(0, len(tiles), 4)])
        seen["scores"] = tl.tile_gate_np(maps, 0.0)[1]
        return maps

    tl.predict_tiled_np(frame, model_fn, 32, 16, 16, 2, "probs", None, 1, "bgr")
    gate = float(np.sort(seen["scores"])[len(seen["scores"]) // 3])               # a score itself: drops a third of the patches
    _, want_out = tl.predict_tiled_np(frame, model_fn, 32, 16, 16, 2, "probs", gate, 1, "bgr")
    plane = want_out[..., 1]
    hi, lo, mean = (float(np.quantile(plane, q)) for q in (0.9, 0.6, 0.75))
    post = dict(thr_high=hi, thr_low=lo, min_area=4, mean_prob_thr=mean)
    want_h, want_f = pm.postprocess_probmap_np(want_out[None], channel=1, **post)
    final, output = frame_loop.process_frames_optimized(m, frame[None], patch_size=32, stride=16, target_size=16, gate_thr=gate, **post)
    assert output.dtype == torch.float32 and tuple(output.shape) == (1, 48, 70, 2) and final.dtype == torch.uint8
    assert np.array_equal(output[0].cpu().numpy().view(np.uint32), want_out.view(np.uint32))
    assert np.array_equal(final.cpu().numpy(), want_f)
    assert want_h.any() and not want_h.all()                  # the thresholds cut through the map


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def test_arguments(torch_cuda, model):
    torch = torch_cuda
    prob = torch.zeros((1, 16, 16), dtype=torch.float32, device="cuda")
    mask = torch.zeros((1, 16, 16), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError) as err:
        pm.hysteresis(model, prob.cpu())
    assert str(err.value) == "prob must be a float32 CUDA tensor [B,H,W] or [B,H,W,C]"
    with pytest.raises(RuntimeError, match="mask must be a uint8 CUDA tensor"):
        pm.filter_by_mean_prob(model, mask.cpu(), prob)
    with pytest.raises(RuntimeError, match="prob must be"):
        pm.threshold_levels(model, prob.double(), 0.5)
    with pytest.raises(ValueError, match="thr_low"):
        pm.hysteresis(model, prob, 0.7, 0.9)
    with pytest.raises(ValueError, match="channel"):
        pm.threshold_levels(model, torch.zeros((1, 4, 4, 2), device="cuda"), 0.5)
    with pytest.raises(ValueError, match="thresholds"):
        pm.threshold_histogram(model, prob, mask, [0.5, 0.5])
    with pytest.raises(ValueError, match="target"):
        pm.threshold_histogram(model, prob, mask[:, :8], [0.5])
    with pytest.raises(ValueError, match="out_value"):
        pm.hysteresis(model, prob, out_value=0)


def test_c_abi_errors_launch_nothing(torch_cuda, model):
    torch = torch_cuda
    from unet_amd import _lib
    lib = _lib.load()
    E_INVALID = -1
    prob = torch.zeros((1, 8, 8), dtype=torch.float32, device="cuda")
    codes = torch.full((1, 8, 8), 9, dtype=torch.uint8, device="cuda")
    counts = torch.full((16,), 7, dtype=torch.int32, device="cuda")
    h, p = model._handle, lambda t: ctypes.c_void_p(t.data_ptr())
    thr = (ctypes.c_float * 2)(0.5, 0.5)
    assert lib.unetpp_probmap_layout(None) == E_INVALID
    assert lib.unetpp_prob_levels_f32(h, p(prob), 1, 0, 1, 8, 8, 0.9, 0.7, p(codes), None) == E_INVALID       # t_low > t_high
    assert lib.unetpp_prob_levels_f32(h, p(prob), 2, 2, 1, 8, 8, 0.5, 0.7, p(codes), None) == E_INVALID       # channel >= stride
    assert lib.unetpp_prob_levels_f32(h, p(prob), 1, 0, 0, 8, 8, 0.5, 0.7, p(codes), None) == E_INVALID       # batch 0
    assert lib.unetpp_prob_levels_f32(h, None, 1, 0, 1, 8, 8, 0.5, 0.7, p(codes), None) == E_INVALID
    assert lib.unetpp_prob_threshold_hist_f32(h, p(prob), 1, 0, p(codes), 1, 8, 8, thr, 2, -1, -1, p(counts), p(counts[8:]), None, None) == E_INVALID
    assert lib.unetpp_prob_threshold_hist_f32(h, p(prob), 1, 0, p(codes), 1, 8, 8, thr, 0, -1, -1, p(counts), p(counts[8:]), None, None) == E_INVALID
    assert lib.unetpp_prob_threshold_hist_f32(h, p(prob), 1, 0, p(codes), 1, 8, 8, thr, 257, -1, -1, p(counts), p(counts[8:]), None, None) == E_INVALID
    assert lib.unetpp_components_prob_sum_f32(h, p(counts), p(prob), 1, 0, 1, 8, 8, 1, p(counts), None) == E_INVALID     # capacity 1
    assert lib.unetpp_components_filter_mean(h, p(counts), p(counts), p(counts), p(counts), 1, 8, 8, 1, 1, 1, 1, p(codes), p(counts), None) == E_INVALID
    torch.cuda.synchronize()
    assert (codes == 9).all() and (counts == 7).all()
