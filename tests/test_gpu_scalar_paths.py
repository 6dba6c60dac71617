"""The scalar side of conv3x3_ws_kernel (csrc/conv3x3_ws.h): arguments read in place by each role, the tile cursor stepped at
the loop's end, one DMA base per chunk, the split-K launches in a kernel of their own.  None of it changes a product or a sum,
so the shapes below are chosen for the PATHS they take, and every case holds the logits to the oracle on the host at the bars
the suite uses for such sizes (exact: 2e-5, exact8: 1e-3, flipped mask pixels only at near-ties of the reference) and asks
for the same bits from a second forward.
Run on the GPU box:  python -m pytest tests -m gpu"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = {"exact": 2e-5, "exact8": 1e-3}      # tests/test_gpu_parity.py, tests/test_gpu_exact8.py


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


_REF = {}


def reference(oracle, syn, C, B, H, W):
    """frames, state dict and the oracle's logits / mask of one shape: computed once, shared by both precisions"""
    key = (C, B, H, W)
    if key not in _REF:
        frames = syn.make_frames_u8(B, H, W, "smooth", 7)
        sd = syn.make_state_dict(C, 3, C == 3, 2)
        ref = oracle.torch_forward(sd, syn.frames_to_chw_f32(frames))
        ref.setflags(write=False)
        _REF[key] = (frames, sd, ref, oracle.masks_from_logits(ref)[0])
    return _REF[key]


def make_model(C, sd, B, hw, precision):
    from unet_amd.nested_unet import NestedUNet
    m = NestedUNet(C, deep_supervision=(C == 3), precision=precision, max_batch=B, max_hw=hw).to("cuda:0")
    m.load_state_dict(sd, strict=True)
    return m.eval()


def gate(tag, precision, logits, mask, ref, ref_mask, oracle):
    err = float(np.abs(logits - ref).max())
    margin = oracle.top2_margin(ref)
    flips = mask != ref_mask
    print(f"{tag} {precision}: max|dlogit|={err:.3e} flips={int(flips.sum())}/{flips.size}")
    assert err < TOL[precision], f"{tag}: logit error {err:.3e}"
    assert not (flips & (margin > 2 * err + 1e-7)).any(), f"{tag}: a flipped pixel is not a near-tie"


# 2 x 64 x 192: the smallest size with interior tiles at level 0 (16-row tiles: rows 16..47, columns 32..159) and level 1
#               (8-row tiles of the 32 x 96 image), i.e. the producers' origin-plus-constant offsets next to border tiles
# 1 x 64 x 96:  one frame: the split-K plan at level 4 (conv3x3_ws_splitk_kernel) and the low-resolution GEMM at levels 2-3
# 2 x 48 x 80, 7 classes: every tile on the border (partial tiles in both directions), the widest head the repository's
#               fixtures use in the fused epilogue
@pytest.mark.parametrize("precision", ["exact", "exact8"])
@pytest.mark.parametrize("C,B,H,W", [(3, 2, 64, 192), (3, 1, 64, 96), (7, 2, 48, 80)])
def test_paths_against_oracle_and_repeatable(C, B, H, W, precision, torch_cuda, syn, oracle):
    torch = torch_cuda
    frames, sd, ref, ref_mask = reference(oracle, syn, C, B, H, W)
    model = make_model(C, sd, B, (H, W), precision)
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    mask, logits = model.segment(x, return_logits=True)
    mask2, logits2 = model.segment(x, return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(logits, logits2) and torch.equal(mask, mask2)          # same launch plan, same bits
    gate(f"C={C} {B}x{H}x{W}", precision, logits.cpu().numpy(), mask.cpu().numpy(), ref, ref_mask, oracle)
    assert model.status() == 0


@pytest.mark.parametrize("precision", ["exact", "exact8"])
def test_first_block_uint8_and_float32_inputs_agree(precision, torch_cuda, syn, oracle):
    """The fused first block reads the caller's tensor itself: uint8 BGR frames and their float32 CHW form give the same
    masks and logits (2 x 64 x 192: interior and border patches)."""
    torch = torch_cuda
    frames, sd, ref, ref_mask = reference(oracle, syn, 3, 2, 64, 192)
    model = make_model(3, sd, 2, (64, 192), precision)
    m_f, l_f = model.segment(torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda(), return_logits=True)
    m_u, l_u = model.segment(torch.from_numpy(frames).cuda(), return_logits=True)
    m_u2, l_u2 = model.segment(torch.from_numpy(frames).cuda(), return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(m_f, m_u) and torch.equal(l_f, l_u)
    assert torch.equal(m_u, m_u2) and torch.equal(l_u, l_u2)
    gate("uint8 input 2x64x192", precision, l_u.cpu().numpy(), m_u.cpu().numpy(), ref, ref_mask, oracle)
    assert model.status() == 0
