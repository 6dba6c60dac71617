"""Connected components and the reference's component filters on the device (unetpp_components,
unetpp_components_filter) against the NumPy restatement (unet_amd/components.py) and the fixtures made from the
reference's own filter functions (tests/golden/cc_*.npz).  Everything is integer: exact equality, no tolerance.
Run on the GPU box:  python -m pytest tests/test_gpu_components.py -m gpu"""
import ctypes
import hashlib

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import components as cc

pytestmark = pytest.mark.gpu

K = 8192
SCENE_TABLE = {      # (H, W, seed, class) -> (components, kept by largest(min_area=50), cable_shape(roi_width=W), spatial)
    (512, 512, 0, 1): (1487, 21511, 21511, 32258), (512, 512, 0, 2): (1386, 38827, 0, 38827),
    (512, 512, 1, 1): (1479, 22276, 22276, 33003), (512, 512, 1, 2): (1462, 37601, 0, 37601),
    (448, 800, 0, 1): (2070, 29434, 0, 44143), (448, 800, 0, 2): (1927, 53028, 0, 53028),
    (448, 800, 1, 1): (2011, 30480, 0, 45197), (448, 800, 1, 2): (1945, 51421, 0, 51421),
}
RULE_KW = {"largest": {"min_area": 50}, "cable_shape": {}, "spatial": {}}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def model(torch_cuda):
    from unet_amd.nested_unet import NestedUNet
    return NestedUNet(3, max_batch=1, max_hw=(16, 16)).to("cuda:0")      # no weights: the components need none


def expected(masks, connectivity, match_class, k=K):
    """labels, num, stats [B,k,5], sums [B,k,2] of the restatement, truncated / zero-padded to k rows."""
    B, H, W = masks.shape
    labels = np.zeros((B, H, W), np.int32)
    num = np.zeros(B, np.int32)
    stats = np.zeros((B, k, 5), np.int32)
    sums = np.zeros((B, k, 2), np.uint64)
    for b in range(B):
        l, s, sm = cc.components_np(masks[b], connectivity, match_class)
        labels[b], num[b] = l, len(s)
        n = min(len(s), k)
        stats[b, :n], sums[b, :n] = s[:n], sm[:n]
    return labels, num, stats, sums


def check_components(torch, model, masks, connectivity, match_class, k=K):
    d = torch.from_numpy(masks).cuda()
    labels, num, stats, cen = model.components(d, match_class=match_class, connectivity=connectivity, max_components=k)
    torch.cuda.synchronize()
    rl, rn, rs, rsum = expected(masks, connectivity, match_class, k)
    assert labels.dtype == torch.int32 and num.dtype == torch.int32 and stats.dtype == torch.int32 and cen.dtype == torch.float64
    assert np.array_equal(num.cpu().numpy(), rn), (num.cpu().numpy(), rn)
    assert np.array_equal(labels.cpu().numpy(), rl)
    assert np.array_equal(stats.cpu().numpy(), rs)
    got_cen, ref_cen = cen.cpu().numpy(), cc.centroids_np(rs, rsum)
    assert np.array_equal(np.isnan(got_cen), np.isnan(ref_cen))
    assert np.array_equal(np.nan_to_num(got_cen), np.nan_to_num(ref_cen))        # one correctly rounded division each
    # the integer sums themselves, through the ABI's uint64 output
    raw = model._components(d, match_class, connectivity, k, True)
    torch.cuda.synchronize()
    assert np.array_equal(raw[3].cpu().numpy().view(np.uint64), rsum)
    return rn


# ---- 1. labels, num, stats, sums against the restatement ------------------------------------------------------
@pytest.mark.parametrize("hw", [(512, 512), (448, 800)])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_scenes_match_restatement(hw, connectivity, torch_cuda, model):
    masks = np.stack([cc.make_scene_mask(hw[0], hw[1], seed) for seed in range(4)])
    for cls in (1, 2):
        num = check_components(torch_cuda, model, masks, connectivity, cls)
        if connectivity == 8:
            assert [int(n) - 1 for n in num[:2]] == [SCENE_TABLE[(hw[0], hw[1], s, cls)][0] for s in range(2)]


@pytest.mark.parametrize("connectivity", [4, 8])
def test_speckled_net_masks_match_restatement(connectivity, torch_cuda, model):
    masks = np.ascontiguousarray(load_golden("b_c3_512x512")["mask"])
    most = 0
    for cls in (0, 1, 2):
        most = max(most, int(check_components(torch_cuda, model, masks, connectivity, cls).max()) - 1)
    check_components(torch_cuda, model, masks, connectivity, -1)
    if connectivity == 4:
        assert most == 3864              # the speckle of class 2 in frame 0: nothing trivial was compared


@pytest.mark.parametrize("hw", [(37, 300), (1, 1), (5, 1027), (33, 129), (1, 4099)])
def test_ragged_sizes_match_restatement(hw, torch_cuda, model):
    r = np.random.default_rng(hw[0] * 10007 + hw[1])
    masks = np.stack([(r.random(hw) < d).astype(np.uint8) * np.uint8(1 + i) for i, d in enumerate((0.2, 0.5, 0.8))])
    for connectivity in (4, 8):
        check_components(torch_cuda, model, masks, connectivity, -1)
        check_components(torch_cuda, model, masks, connectivity, 2)
    check_components(torch_cuda, model, np.ones((1,) + hw, np.uint8), 8, 1)


# ---- 2. adversarial shapes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
def test_adversarial_shapes(connectivity, torch_cuda, model):
    adv = cc.make_adversarial_masks(512, 512)
    names = [n for n in adv if n != "checkerboard"]
    num = check_components(torch_cuda, model, np.stack([adv[n] for n in names]), connectivity, 1)
    got = dict(zip(names, (int(n) - 1 for n in num)))
    diag = 1 if connectivity == 8 else 512
    assert got == {"ones": 1, "zeros": 0, "serpentine": 1, "comb": 1, "diagonal": diag, "antidiagonal": diag, "tile_corners": 85}


def test_checkerboard_beyond_capacity(torch_cuda, model):
    torch = torch_cuda
    board = cc.make_adversarial_masks(512, 512)["checkerboard"][None]
    assert int(check_components(torch, model, board, 8, 1)[0]) == 2
    num = check_components(torch, model, board, 4, 1)            # num exact, the first K stats rows right
    assert int(num[0]) == 512 * 512 // 2 + 1 > K
    d = torch.from_numpy(board).cuda()
    with pytest.raises(RuntimeError, match=rf"frame 0 .*{512 * 512 // 2 + 1}.*{K}"):
        model.filter_components(d, 1, rule="largest", connectivity=4, min_area=0)
    out = model.filter_components(d, 1, rule="largest", connectivity=4, min_area=0, check=False)
    assert int(out.count_nonzero()) == 0                          # undecidable from truncated stats: nothing kept
    both = torch.from_numpy(np.concatenate([board, board])).cuda()
    kept = model.filter_components(both, 1, rule="largest", connectivity=8, min_area=0, max_components=2)
    assert np.array_equal(kept.cpu().numpy(), np.concatenate([board, board]))


# ---- 3. reproducible bit for bit ---------------------------------------------------------------------------------
def test_same_bits_run_to_run_and_on_a_second_stream(torch_cuda, model):
    torch = torch_cuda
    adv = cc.make_adversarial_masks(512, 512)
    masks = np.stack([cc.make_scene_mask(512, 512, 0), cc.make_scene_mask(512, 512, 1), adv["serpentine"], adv["comb"],
                      np.ascontiguousarray(load_golden("b_c3_512x512")["mask"][0])])
    d = torch.from_numpy(masks).cuda()
    runs = [model._components(d, 1, 8, K, True)[:4] for _ in range(2)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runs.append(model._components(d, 1, 8, K, True)[:4])
    side.synchronize()
    torch.cuda.synchronize()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


# ---- 4. the three filters against the reference's own functions ----------------------------------------------------
@pytest.mark.parametrize("name", ["cc_scenes", "cc_net_masks"])
def test_filters_match_the_references_functions(name, torch_cuda, model):
    torch = torch_cuda
    g = load_golden(name)
    net = np.ascontiguousarray(load_golden("b_c3_512x512")["mask"]) if name == "cc_net_masks" else None
    kept_any = {rule: 0 for rule in RULE_KW}
    for tag, H, W, which, cls, sha in (tuple(r) for r in g["cases"].tolist()):
        H, W, which, cls = int(H), int(W), int(which), int(cls)
        mask = cc.make_scene_mask(H, W, which) if net is None else net[which]
        assert hashlib.sha256(mask.tobytes()).hexdigest() == sha
        d = torch.from_numpy(mask[None]).cuda()
        labels, num, stats, cen = model.components(d, cls)
        assert int(num[0]) == int(g[tag + "_num"])
        assert np.array_equal(stats[0, :64].cpu().numpy(), g[tag + "_stats"])
        assert np.array_equal(cen[0, 1:64].cpu().numpy(), g[tag + "_centroids"][1:64])
        for i, (rule, kw) in enumerate(RULE_KW.items()):
            out_value = 255 if rule == "cable_shape" else 1
            got = model.filter_components(d, cls, rule=rule, out_value=out_value, **kw)[0].cpu().numpy()
            ref = np.unpackbits(g[f"{tag}_{rule}"])[:H * W].reshape(H, W)
            assert got.dtype == np.uint8 and np.array_equal(got, ref * np.uint8(out_value)), (tag, rule)
            assert np.array_equal(got, cc.filter_components_np(mask, cls, rule, out_value=out_value, **kw))
            kept_any[rule] += int(ref.sum())
            if net is None:
                assert int((got != 0).sum()) == SCENE_TABLE[(H, W, which, cls)][1 + i], (tag, rule)
    if net is None:
        assert all(v > 0 for v in kept_any.values())              # no rule was compared on empty masks only


def test_filters_batched_with_other_parameters(torch_cuda, model):
    torch = torch_cuda
    masks = np.stack([cc.make_scene_mask(448, 800, seed) for seed in range(3)] + [np.zeros((448, 800), np.uint8)])
    d = torch.from_numpy(masks).cuda()
    cases = [("largest", {"min_area": 0}), ("largest", {"min_area": 10 ** 6}), ("spatial", {"min_width": 20, "max_width": 400, "min_height_ratio": 0.1, "min_area": 5}),
             ("cable_shape", {"roi_width": 400, "min_aspect": 1.2, "max_center_offset": 0.45, "min_area": 200}),
             ("cable_shape", {"roi_width": 1200.5, "min_aspect": 1.0, "max_center_offset": 2.0, "min_area": 2})]
    for cls in (1, 2, -1):
        for connectivity in (4, 8):
            for rule, kw in cases:
                got = model.filter_components(d, cls, rule=rule, connectivity=connectivity, out_value=7, **kw).cpu().numpy()
                ref = np.stack([cc.filter_components_np(m, cls, rule, connectivity, 7, **kw) for m in masks])
                assert np.array_equal(got, ref), (cls, connectivity, rule, kw)


# ---- 5. end to end -------------------------------------------------------------------------------------------------
def test_segment_filter_mask_stats_end_to_end(torch_cuda, syn, oracle):
    torch = torch_cuda
    from unet_amd.nested_unet import NestedUNet
    g = load_golden("b_c3_512x512")
    kinds = [str(k) for k in g["kinds"]]
    frames = np.stack([syn.make_frame_u8(512, 512, i, kinds[i % len(kinds)], int(g["fseed"])) for i in range(int(g["B"]))])
    net = NestedUNet(3, deep_supervision=True, max_batch=2, max_hw=(512, 512)).to("cuda:0")
    net.load_state_dict(syn.make_state_dict(3, 3, True, int(g["wseed"])), strict=True)
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    mask = net.eval().segment(x)
    before = mask.clone()
    for cls, min_area in ((1, 50), (2, 50), (2, 0)):
        kept = net.filter_components(mask, match_class=cls, rule="largest", min_area=min_area)
        counts, widths = net.mask_stats(kept)
        torch.cuda.synchronize()
        host = mask.cpu().numpy()
        ref_kept = np.stack([cc.filter_components_np(m, cls, "largest", min_area=min_area) for m in host])
        assert np.array_equal(kept.cpu().numpy(), ref_kept) and ref_kept.any()
        ref_counts, ref_widths = oracle.mask_stats_np(ref_kept, 3)
        assert np.array_equal(counts.cpu().numpy(), ref_counts)
        assert np.array_equal(widths.cpu().numpy(), ref_widths)
    assert net.status() == 0
    assert torch.equal(net.segment(x), before)


def test_simple_unet_inherits_the_methods(torch_cuda):
    torch = torch_cuda
    from unet_amd.nested_unet import SimpleUNet
    m = SimpleUNet(3).to("cuda:0")
    mask = cc.make_scene_mask(64, 96, 3, noise=0.1)[None]
    got = m.filter_components(torch.from_numpy(mask).cuda(), 2, rule="largest", min_area=0)
    assert np.array_equal(got[0].cpu().numpy(), cc.filter_components_np(mask[0], 2, "largest", min_area=0))


# ---- 6. the C ABI's error returns ----------------------------------------------------------------------------------
def test_c_abi_error_returns(torch_cuda, model):
    torch = torch_cuda
    from unet_amd import _lib
    lib = _lib.load()
    B, H, W = 1, 32, 48
    model.components(torch.zeros((B, H, W), dtype=torch.uint8, device="cuda"))       # makes sure the engine exists
    h = model._handle
    mask = torch.zeros((B, H, W), dtype=torch.uint8, device="cuda")
    labels = torch.empty((B, H, W), dtype=torch.int32, device="cuda")
    num = torch.empty((B,), dtype=torch.int32, device="cuda")
    stats = torch.empty((B, 16, 5), dtype=torch.int32, device="cuda")
    sums = torch.empty((B, 16, 2), dtype=torch.int64, device="cuda")
    out = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
    nbytes = lib.unetpp_components_workspace_bytes(B, H, W, 16)
    assert nbytes >= B * H * W * 4 + 16
    assert lib.unetpp_components_workspace_bytes(B, H, W, 1) == 0 and lib.unetpp_components_workspace_bytes(0, H, W, 16) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    err = lambda: lib.unetpp_last_error(h).decode()

    def run(mask_=mask, conn=8, cap=16, labels_=labels, num_=num, stats_=stats, sums_=sums, ws_=ws, b=B, hh=H, ww=W):
        return lib.unetpp_components(h, p(mask_), b, hh, ww, 1, conn, cap, p(labels_), p(num_), p(stats_), p(sums_), p(ws_), None)

    assert run() == 0
    assert run(conn=6) == -1 and "connectivity" in err()
    assert run(cap=1) == -1 and "capacity" in err()
    assert run(labels_=None) == -1 and "null" in err()
    assert run(mask_=None) == -1 and run(num_=None) == -1 and run(ws_=None) == -1
    assert run(stats_=None) == -1 and "both or neither" in err()
    assert run(stats_=None, sums_=None) == 0                     # labels and num only
    assert run(hh=0) == -1 and "shape" in err()
    assert lib.unetpp_components(None, p(mask), B, H, W, 1, 8, 16, p(labels), p(num), p(stats), p(sums), p(ws), None) == -1
    rule = _lib.CcRule(0.0, 50.0, 300.0, 0.3, 1.6, 0.3, float(W))

    def filt(labels_=labels, rule_id=0, cap=16, params=rule, out_=out):
        return lib.unetpp_components_filter(h, p(labels_), p(num), p(stats), p(sums), B, H, W, cap, rule_id,
                                            ctypes.byref(params) if params is not None else None, 1, p(out_), p(ws), None)

    assert run() == 0 and filt() == 0
    assert filt(rule_id=3) == -1 and "rule" in err()
    assert filt(cap=1) == -1 and "capacity" in err()
    assert filt(labels_=None) == -1 and filt(out_=None) == -1 and filt(params=None) == -1
    assert filt(rule_id=2, params=_lib.CcRule(0.0, 50.0, 300.0, 0.3, 1.6, 0.3, 0.0)) == -1 and "roi_width" in err()
    torch.cuda.synchronize()
    assert int(num[0]) == 1 and int(out.count_nonzero()) == 0
