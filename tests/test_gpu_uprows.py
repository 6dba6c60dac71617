"""conv3x3_ws_uprows_kernel (csrc/conv3x3_ws.h, UR): conv0_4.conv1 of `exact` with its up chunks multiplied on low-resolution rows
and interpolated in y afterwards.  Against the CPU oracle, against the plain fused-upsample kernel of the same build (the
route debug_keep_intermediates takes for this layer) and for batch-row invariance.  Run on the GPU box: python -m pytest tests -m gpu"""
import numpy as np
import pytest

from test_gpu_parity import make_model, report, torch_cuda  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

# 16 x 32: one tile with both image borders; 48 x 80: a middle row tile and a partial column tile; 80 x 48: the transposed case
CASES = [(3, 1, 16, 32), (3, 2, 48, 80), (3, 1, 80, 48), (3, 3, 32, 96), (7, 1, 48, 80)]


@pytest.mark.parametrize("C,B,H,W", CASES, ids=lambda v: str(v))
def test_uprows_against_oracle_plain_kernel_and_row_order(C, B, H, W, torch_cuda, syn, oracle):
    torch = torch_cuda
    frames = syn.make_frames_u8(B, H, W, "smooth", 100 * H + W)
    x = syn.frames_to_chw_f32(frames)
    model, sd = make_model(C, C == 3, 11, "exact", syn, B, (H, W))
    ref = oracle.torch_forward(sd, x)
    xt = torch.from_numpy(x).cuda()

    model(xt)                                              # creates the engine
    model.profile(True)
    mask, logits = model.segment(xt, return_logits=True)
    torch.cuda.synchronize()
    names = [r[0] for r in model.profile_read()]
    model.profile(False)
    assert any(n.startswith("conv0_4.conv1+up|conv3x3_ws_uprows_kernel") for n in names), names

    # the random-shape sweep's bar (test_gpu_parity.test_random_shapes_against_oracle)
    err, flips, unexplained = report(logits.cpu().numpy(), mask.cpu().numpy(), ref, oracle.masks_from_logits(ref)[0], oracle)
    scale = max(1.0, float(np.abs(ref).max()))
    print(f"uprows {C}c {B}x{H}x{W}: max|dlogit|={err:.3e} scale={scale:.3f} flips={flips} unexplained={unexplained}")
    assert err < 2e-5 * scale and unexplained == 0, (err, scale, flips)

    # today's kernel for this layer, same build: two plans of one layer differ in rounding only -- and do differ
    model.debug_keep_intermediates(True)
    plain = model(xt)
    torch.cuda.synchronize()
    model.debug_keep_intermediates(False)
    d = float((plain - logits).abs().max())
    print(f"uprows vs plain fused-upsample kernel: max|dlogit|={d:.3e}")
    assert 0 < d < 5e-6, d

    # a frame's result does not depend on its row of the batch: the permuted batch, row for row, bit for bit
    perm = torch.arange(B - 1, -1, -1, device=xt.device)
    again = model(xt[perm].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(again, logits[perm])
