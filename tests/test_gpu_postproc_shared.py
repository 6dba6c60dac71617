"""The input check and the call that every post-processing method shares (unet_amd/postproc.py), on the device: each path
into them as the FIRST call of a fresh model (no .to(), no forward: the check adopts the tensor's device and builds the
engine), once with a strided view and once with its contiguous copy -- bitwise the same results -- and the refusal of a
tensor on another device before any engine exists.
Run on the GPU box:  python -m pytest tests/test_gpu_postproc_shared.py -m gpu"""
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def weights(syn):
    return syn.make_state_dict(3, 3, True, 0)


@pytest.fixture(scope="module")
def views(torch_cuda):
    """Non-contiguous views, every second column of a tensor twice as wide, at the smallest shapes every entry accepts."""
    torch = torch_cuda
    g = torch.Generator().manual_seed(0)
    rand = lambda hi, shape, dtype: torch.randint(0, hi, shape, generator=g).to(dtype).cuda()
    return {"mask": rand(3, (2, 16, 48), torch.uint8)[:, :, ::2],                  # class indices [2,16,24]
            "gray": rand(256, (2, 16, 48), torch.uint8)[:, :, ::2],
            "frames": rand(256, (2, 16, 48, 3), torch.uint8)[:, :, ::2],           # [2,16,24,3]
            "widths": rand(40, (2, 2, 32), torch.float32)[:, :, ::2],              # [2,2,16]
            "maps": (rand(1000, (2, 3, 16, 32), torch.float32) / 1000)[:, :, :, ::2],      # [2,3,16,16]
            "num": torch.tensor([3, 9, 2, 9], dtype=torch.int32).cuda()[::2],      # [2]
            "stats": rand(50, (2, 8, 5), torch.int32)[:, ::2]}                     # [2,4,5]


CALLS = {
    "mask_stats": lambda m, v: m.mask_stats(v["mask"]),
    "components": lambda m, v: m.components(v["mask"], 1, max_components=64),
    "morphology": lambda m, v: m.morphology(v["mask"], 1),
    "row_widths": lambda m, v: m.row_widths(v["mask"], 1, v["mask"], 2),
    "width_profile": lambda m, v: m.width_profile(v["widths"]),
    "components_summary": lambda m, v: m.components_summary(v["num"], v["stats"]),
    "count_nonzero": lambda m, v: m.count_nonzero(v["mask"]),
    "clahe": lambda m, v: m.clahe(v["gray"], tile_grid=(2, 2)),
    "resize_frames": lambda m, v: m.resize_frames(v["frames"], (8, 8)),
    "resize_masks": lambda m, v: m.resize_masks(v["mask"], (8, 8)),
    "tile_gate": lambda m, v: m.tile_gate(v["maps"], 0.5),
}


def bits(result):
    """dtype, shape and bytes of every tensor of a result (NaN centroids compare as bytes)."""
    result = result if isinstance(result, (tuple, list)) else (result,)
    return [None if t is None else (t.dtype, tuple(t.shape), t.cpu().numpy().tobytes()) for t in result]


@pytest.mark.parametrize("name", list(CALLS))
def test_first_call_on_a_fresh_model_takes_a_strided_view(name, torch_cuda, weights, views):
    from unet_amd.nested_unet import NestedUNet
    model = NestedUNet(3, max_batch=2, max_hw=(32, 32))
    model.load_state_dict(weights, strict=True)
    assert model._handle is None and model._device_index is None
    assert not any(t.is_contiguous() for t in views.values())
    strided = bits(CALLS[name](model, views))
    assert model._handle is not None and model._device_index == views["mask"].device.index
    assert bits(CALLS[name](model, {k: t.contiguous() for k, t in views.items()})) == strided


def test_a_tensor_on_another_device_is_refused_before_any_engine_exists(torch_cuda, views):
    from unet_amd.nested_unet import NestedUNet
    model = NestedUNet(3).to("cuda:1")                    # records the index, touches no device
    v = {k: t.contiguous() for k, t in views.items()}
    for call in (lambda: model.mask_stats(v["mask"]), lambda: model.resize_frames(v["frames"], (8, 8)),
                 lambda: model.resize_masks(v["mask"], (8, 8)), lambda: model.components_summary(v["num"], None)):
        with pytest.raises(RuntimeError, match="on cuda:0, engine on cuda:1"):
            call()
    assert model._handle is None
