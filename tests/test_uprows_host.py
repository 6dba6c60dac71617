"""The row identity behind conv3x3_ws_uprows_kernel (csrc/conv3x3_ws.h, UR), on the host in float64.

The x2 bilinear upsample (align_corners=True) is separable, U[y'] = (1 - f(y')) T[r(y')] + f(y') T[r(y') + 1] with T the
x-interpolation of a low row, so the up half of a fused-upsample conv is a fold of 1x3 products on LOW rows,
    S[y] = sum_dy [0 <= y + dy < H] ((1 - f) Y_dy[r(y + dy)] + f Y_dy[r(y + dy) + 1]),   Y_dy[r][x] = sum_dx W[dy, dx] T[r][x + dx].
The kernel's wave plan (16-row tiles, k0 = y0 / 2, wave w owns low rows k0 + 2 w, k0 + 2 w + 1, waves 0 / 3 also k0 - 1 / k0 + 8,
four accumulators come from the neighbours) is restated here as small Python functions next to the C++ ones."""
import numpy as np
import pytest

NCONS, MW, TH, TW = 4, 4, 16, 32


def ur_row(m, dy):
    """low row of image row 4 w + m + dy relative to k0 + 2 w (conv3x3_ws.h ur_row): -1 .. 2"""
    return (m + dy + 1) // 2 - 1


def owned(w):
    """(dy, l) pairs wave w accumulates itself, l relative to k0 + 2 w"""
    own = {(dy, l) for dy in (-1, 0, 1) for l in (0, 1)}
    if w == 0:
        own |= {(-1, -1), (0, -1)}
    if w == NCONS - 1:
        own |= {(0, 2), (1, 2)}
    return own


def received(w):
    """the four (dy, l) pairs wave w takes out of the exchange: two from each neighbour it has"""
    got = set()
    if w > 0:
        got |= {(-1, -1), (0, -1)}          # rows k0 + 2 w - 1 of wave w - 1
    if w < NCONS - 1:
        got |= {(0, 2), (1, 2)}             # rows k0 + 2 w + 2 of wave w + 1
    return got


def ac_rows_f32(n_out):
    """(source coordinate, lower source row, fraction) of every output row in float32, as the kernels compute them: an odd row takes
    the lower source row of the even row after it (its 2x2 block partner) while that one is inside the image"""
    n_in = n_out // 2
    s = np.float32(n_in - 1) / np.float32(n_out - 1) if n_in > 1 else np.float32(0)
    y = np.arange(n_out)
    src = (s * y.astype(np.float32)).astype(np.float32)
    partner = np.where((y % 2 == 1) & (y + 1 < n_out), y + 1, y)
    i0 = np.minimum(src[partner].astype(np.int32), n_in - 1)
    f = np.clip(src - i0.astype(np.float32), np.float32(0), np.float32(1))
    return src, i0, f


def plan_row(y):
    """the low row the wave plan assigns to image row y: rows 2 k + 1 and 2 k + 2 read low rows k and k + 1"""
    return (y + 1) // 2 - 1 if y > 0 else 0 if y == 0 else -1


@pytest.mark.parametrize("H", list(range(16, 4097, 16)))
def test_plan_rows_are_the_kernels_rows_and_every_read_is_owned_or_received(H):
    src, i0, f = ac_rows_f32(H)
    assert np.array_equal(i0, [plan_row(y) for y in range(H)])
    src, i0, f = src.tolist(), i0.tolist(), f.tolist()       # (float32 values as Python floats: src - r below is exact in both)
    assert f[0] == 0 and f[H - 1] == 0            # the last row's second source row (outside the low image) has weight 0
    for y0 in range(0, H, TH):
        k0 = y0 // 2
        for w in range(NCONS):
            have = owned(w) | received(w)
            assert not (owned(w) & received(w)) and len(received(w)) == (4 if 0 < w < NCONS - 1 else 2)
            for m in range(MW):
                for dy in (-1, 0, 1):
                    yy = y0 + MW * w + m + dy
                    l = ur_row(m, dy)
                    assert (dy, l) in have and (dy, l + 1) in have
                    if 0 <= yy < H:
                        # the fold's fraction, relative to the plan's row, blends the rows the loader blends today (image row 0
                        # sits in the pair (-1, 0) with fraction 1: all of its weight on low row 0)
                        r = k0 + 2 * w + l
                        fr = min(max(src[yy] - r, 0.0), 1.0)
                        assert (r == i0[yy] and fr == f[yy]) or (yy == 0 and r == -1 and fr == 1 and f[yy] == 0)
    # what a wave hands over is what its neighbour owns
    for w in range(NCONS):
        for dy, l in received(w):
            nb = w - 1 if l < 0 else w + 1
            assert (dy, l + 2 * (w - nb)) in owned(nb)


def _x_interp(low, W):
    """T: every low row interpolated to W columns, float64"""
    w = low.shape[-1]
    src = np.arange(W, dtype=np.float64) * ((w - 1) / (W - 1))
    i0 = np.minimum(src.astype(np.int64), w - 1)
    i1 = np.minimum(i0 + 1, w - 1)
    fx = src - i0
    return low[..., i0] * (1 - fx) + low[..., i1] * fx


def fold(low, wgt, H, W):
    """conv3x3(up(low)) by the identity, tile by tile and wave by wave: each wave uses only the Y it owns or receives"""
    cout, cin = wgt.shape[:2]
    h = H // 2
    T = np.zeros((cin, h + 2, W + 2))                 # low rows -1 .. h, columns -1 .. W: zeros outside the image
    T[:, 1:h + 1, 1:W + 1] = _x_interp(low, W)
    src = np.arange(H, dtype=np.float64) * ((h - 1) / (H - 1))
    out = np.zeros((cout, H, W))

    def y_of(dy, r, x0, x1):
        """Y_dy[r][x0:x1] = sum_dx W[dy, dx] T[r][x + dx], zero rows outside the low image"""
        if not -1 <= r <= h:
            return np.zeros((cout, x1 - x0))
        acc = np.zeros((cout, x1 - x0))
        for dx in (-1, 0, 1):
            acc += wgt[:, :, dy + 1, dx + 1] @ T[:, r + 1, x0 + dx + 1:x1 + dx + 1]
        return acc

    for y0 in range(0, H, TH):
        k0 = y0 // 2
        for x0 in range(0, W, TW):
            x1 = min(x0 + TW, W)
            mine = [{(dy, l): y_of(dy, k0 + 2 * w + l, x0, x1) for dy, l in owned(w)} for w in range(NCONS)]
            for w in range(NCONS):
                Y = dict(mine[w])
                for dy, l in received(w):
                    nb = w - 1 if l < 0 else w + 1
                    Y[(dy, l)] = mine[nb][(dy, l + 2 * (w - nb))]
                for m in range(MW):
                    y = y0 + MW * w + m
                    z = np.zeros((cout, x1 - x0))
                    for dy in (-1, 0, 1):                         # fixed order: dy = -1, 0, +1, lower row first
                        yy = y + dy
                        if not 0 <= yy < H:
                            continue
                        l = ur_row(m, dy)
                        f = src[yy] - (k0 + 2 * w + l)
                        z += (1 - f) * Y[(dy, l)]
                        z += f * Y[(dy, l + 1)]
                    out[:, y, x0:x1] = z
    return out


@pytest.mark.parametrize("H,W", [(16, 32), (32, 32), (48, 80), (80, 48)])
def test_fold_equals_conv_of_upsampled(H, W):
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(H * 1000 + W)
    low = rng.standard_normal((3, H // 2, W // 2))
    wgt = rng.standard_normal((2, 3, 3, 3))
    up = F.interpolate(torch.from_numpy(low)[None], scale_factor=2, mode="bilinear", align_corners=True)
    ref = F.conv2d(up, torch.from_numpy(wgt), padding=1)[0].numpy()
    got = fold(low, wgt, H, W)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
