"""CPU side of the deep-supervision outputs: the heads' blob and its size in the C ABI, the strict state-dict
behaviour with and without ds heads, the `output` argument checks, the reference fixtures against the oracle's
restatement, and the engine's interpolation index rule against ATen's tables.  No compute call reaches a GPU."""
import hashlib

import numpy as np
import pytest

from conftest import load_golden

DS = (("ds1_3", "x1_3", 64), ("ds2_2", "x2_2", 128), ("ds3_1", "x3_1", 256))      # output k = 1, 2, 3


def test_ds_blob_layout_and_size(syn):
    from unet_amd import _lib, packing
    lib = _lib.load()
    for C in (1, 3, 7, 8):
        sd = syn.make_state_dict(C, 3, True, 4)
        blob = packing.build_ds_blob(sd, C)
        assert blob.nbytes == lib.unetpp_ds_blob_bytes(C) == 32 + 4 * C * (256 + 128 + 64 + 3)
        hdr = blob[:32].view(np.uint32)
        assert hdr.tolist() == [packing.DS_BLOB_MAGIC, 1, C, 3, 0, 0, 0, 0]
        assert blob[:4].tobytes() == b"UNDS"
        pay = blob[32:].view(np.float32)
        off = 0
        for name, cx in (("ds3_1", 256), ("ds2_2", 128), ("ds1_3", 64)):      # definition order
            assert np.array_equal(pay[off:off + C * cx], sd[name + ".weight"].reshape(-1)); off += C * cx
            assert np.array_equal(pay[off:off + C], sd[name + ".bias"]); off += C
        assert off == pay.size
    assert lib.unetpp_ds_blob_bytes(0) == 0


def test_strict_keys_with_and_without_ds_heads(syn):
    from unet_amd import packing
    from unet_amd.nested_unet import NestedUNet
    sd = syn.make_state_dict(3, 3, True, 1)
    m = NestedUNet(3, deep_supervision=True)
    m.load_state_dict(sd, strict=True)
    assert np.array_equal(m._ds_blob, packing.build_ds_blob(sd, 3))
    missing = {k: v for k, v in sd.items() if not k.startswith("ds1_3.")}
    with pytest.raises(RuntimeError, match="Missing key.*ds1_3.weight"):
        NestedUNet(3, deep_supervision=True).load_state_dict(missing, strict=True)
    with pytest.raises(RuntimeError, match="Missing key"):
        NestedUNet(3, deep_supervision=True).load_state_dict(missing, strict=False)
    with pytest.raises(RuntimeError, match="Unexpected key.*ds3_1"):
        NestedUNet(3, deep_supervision=False).load_state_dict(sd, strict=True)
    m2 = NestedUNet(3, deep_supervision=False)
    _, unexpected = m2.load_state_dict(sd, strict=False)
    assert sorted(unexpected) == sorted(k for k in sd if k.startswith("ds"))
    assert m2._ds_blob is None
    bad = dict(sd)
    bad["ds2_2.weight"] = np.zeros((3, 64, 1, 1), np.float32)
    with pytest.raises(RuntimeError, match="size mismatch for ds2_2.weight"):
        NestedUNet(3, deep_supervision=True).load_state_dict(bad, strict=True)


def test_output_argument_is_checked_before_any_device_work(syn):
    """A model without ds heads and SimpleUNet refuse output != 0 with a clear error (no GPU needed to get there)."""
    from unet_amd.nested_unet import NestedUNet, SimpleUNet
    x = np.zeros((1, 3, 32, 32), np.float32)
    m = NestedUNet(3, deep_supervision=False)
    for call in (lambda: m.forward(x, output=1), lambda: m.segment(x, output=2), lambda: m.predict_proba(x, output=3),
                 lambda: m.segment_thresholded(x, output=1), lambda: m.forward_deep_supervision(x)):
        with pytest.raises(ValueError, match="deep_supervision=False"):
            call()
    md = NestedUNet(3, deep_supervision=True)
    for bad in (4, -1, 1.5, "1", True):
        with pytest.raises(ValueError, match="output must be"):
            md.forward(x, output=bad)
    s = SimpleUNet(7)
    with pytest.raises(NotImplementedError, match="NestedUNet only"):
        s.segment(x, output=1)
    with pytest.raises(NotImplementedError, match="NestedUNet only"):
        s.forward_deep_supervision(x)


@pytest.mark.parametrize("tag", ["ds_c3_64x64", "ds_c7_48x80"])
def test_fixtures_agree_with_oracle_restatement(tag, syn, oracle):
    """The reference's deep-supervision list equals the oracle's CPU graph + 1x1 head + ONE align_corners interpolation."""
    import torch
    import torch.nn.functional as F
    torch.set_num_threads(8)                 # the thread count the fixtures were made with
    g = load_golden(tag)
    C, B, H, W = int(g["num_classes"]), int(g["B"]), int(g["H"]), int(g["W"])
    frames = syn.make_frames_u8(B, H, W, str(g["kind"]), int(g["fseed"]))
    assert hashlib.sha256(frames.tobytes()).hexdigest() == str(g["frames_sha"])
    sd = syn.make_state_dict(C, 3, True, int(g["wseed"]))
    wsha = hashlib.sha256(np.concatenate([v.ravel().astype(np.float64) for v in sd.values()]).tobytes()).hexdigest()
    assert wsha == str(g["weights_sha"])
    logits, t = oracle.torch_forward(sd, syn.frames_to_chw_f32(frames), return_intermediates=True)
    np.testing.assert_allclose(logits, g["out0"], rtol=0, atol=1e-5)
    for k, (head, node, cx) in enumerate(DS, start=1):
        assert t[node].shape[1] == cx
        low = F.conv2d(torch.from_numpy(t[node]), torch.from_numpy(sd[head + ".weight"]), torch.from_numpy(sd[head + ".bias"]))
        assert low.shape[2:] == (H >> k, W >> k)
        ref = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=True).numpy()
        np.testing.assert_allclose(ref, g[f"out{k}"], rtol=0, atol=1e-5, err_msg=f"out{k}")
        assert np.array_equal(g[f"mask{k}"], np.argmax(g[f"out{k}"], axis=1).astype(np.uint8))
        srt = np.sort(g[f"out{k}"], axis=1)
        np.testing.assert_array_equal(g[f"margin{k}"], srt[:, -1] - srt[:, -2])


def _device_axis_table(n_in, n_out):
    """ds_upsample_kernel's index and weight arithmetic, restated in float32 (no contraction): s is the host's
    float(in-1)/float(out-1), src = s * dst, i0 = min(int(src), in-1), i1 = i0 + (i0 < in-1), l1 = clamp(src - i0, 0, 1)."""
    s = np.float32(n_in - 1) / np.float32(n_out - 1)
    src = (s * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = np.clip(src - i0.astype(np.float32), np.float32(0), np.float32(1)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    return i0, i1, l0, l1


def test_device_index_rule_equals_aten_tables(oracle):
    """For every level k = 1..3 and every extent that is a multiple of 16 up to 2048: the weight each output sample gives
    each input sample, read off ATen's F.interpolate(one-hot inputs), equals the rule's exactly.  This pins the RULE (the
    restatement above); that ds_upsample_kernel computes it, with two roundings and no contraction, is pinned on the device
    by tests/test_gpu_deep_supervision.py::test_upsample_kernel_pinned_apart_from_the_trunk."""
    import torch
    import torch.nn.functional as F
    for n_out in range(16, 2049, 16):
        for k in (1, 2, 3):
            n_in = n_out >> k
            i0, i1, l0, l1 = _device_axis_table(n_in, n_out)
            r0, r1, q0, q1 = oracle.bilinear_axis_tables(n_in, n_out)
            assert np.array_equal(i0, r0) and np.array_equal(i1, r1) and np.array_equal(l0, q0) and np.array_equal(l1, q1)
            eye = torch.eye(n_in, dtype=torch.float32).reshape(n_in, 1, 1, n_in)
            aten = F.interpolate(eye, size=(1, n_out), mode="bilinear", align_corners=True)[:, 0, 0, :].numpy()
            mine = np.zeros((n_in, n_out), np.float32)
            cols = np.arange(n_out)
            mine[i0, cols] += l0
            mine[i1, cols] += l1
            assert np.array_equal(mine, aten), (n_in, n_out)
