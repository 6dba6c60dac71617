"""The balanced wave plan of conv3x3_ws_uprows_kernel (csrc/conv3x3_ws.h, UR), on the host in float64.

tests/test_uprows_host.py holds the row identity and the first plan (waves 0 and 3 own both accumulators of their edge row: 8, 6, 6,
8).  The kernel now gives every consumer wave ONE of the four edge accumulators, seven each:
    wave 0: (k0 - 1; dy -1)    wave 1: (k0 - 1; dy 0)    wave 2: (k0 + 8; dy 0)    wave 3: (k0 + 8; dy +1)
Wave w writes edge slot w; waves 0 and 3 read the two slots of their side in the fold as before, the inner boundaries exchange four
accumulators as before.  This file restates that plan and folds over it."""
import numpy as np
import pytest

from test_uprows_host import NCONS, MW, TH, TW, _x_interp, ur_row


def edge_owned(w):
    """the edge accumulator of wave w as (dy, low row relative to k0): rows k0 - 1 (waves 0, 1) and k0 + 8 (waves 2, 3)"""
    return [(-1, -1), (0, -1), (0, 2 * NCONS), (1, 2 * NCONS)][w]


def owned(w):
    """(dy, r) pairs wave w accumulates itself, r relative to k0 (absolute within the tile, so that edge rows can sit anywhere)"""
    return {(dy, 2 * w + l) for dy in (-1, 0, 1) for l in (0, 1)} | {edge_owned(w)}


def received(w):
    """(dy, r) pairs wave w takes out of the exchange slots of its inner boundaries"""
    got = set()
    if w > 0:
        got |= {(-1, 2 * w - 1), (0, 2 * w - 1)}
    if w < NCONS - 1:
        got |= {(0, 2 * w + 2), (1, 2 * w + 2)}
    return got


def edge_read(w):
    """(dy, r) pairs wave w reads from the four edge slots behind the scale / bias table"""
    if w == 0:
        return {(-1, -1), (0, -1)}
    if w == NCONS - 1:
        return {(0, 2 * NCONS), (1, 2 * NCONS)}
    return set()


def test_every_wave_owns_seven_and_nobody_owns_a_pair_twice():
    every = [p for w in range(NCONS) for p in sorted(owned(w))]
    assert all(len(owned(w)) == 7 for w in range(NCONS))
    assert len(every) == len(set(every)) == 28
    assert {edge_owned(w) for w in range(NCONS)} == edge_read(0) | edge_read(NCONS - 1)
    # the rows of T a wave multiplies: its own two and one of the tile's first / last (T has rows k0 - 1 .. k0 + 8)
    for w in range(NCONS):
        assert {r for _, r in owned(w)} == {2 * w, 2 * w + 1, -1 if 2 * w < NCONS else 2 * NCONS}


def test_every_read_is_owned_received_or_an_edge_slot():
    for w in range(NCONS):
        have = owned(w) | received(w) | edge_read(w)
        for m in range(MW):
            for dy in (-1, 0, 1):
                r = 2 * w + ur_row(m, dy)
                assert (dy, r) in have and (dy, r + 1) in have, (w, m, dy)
        # what comes out of a slot is owned by exactly one other wave (or, edge slots, possibly by the reader itself)
        for p in received(w):
            assert sum(p in owned(v) for v in range(NCONS) if v != w) == 1 and p not in owned(w)
        for p in edge_read(w):
            assert sum(p in owned(v) for v in range(NCONS)) == 1


def fold(low, wgt, H, W):
    """conv3x3(up(low)) tile by tile and wave by wave: each wave uses only the Y it owns, receives or reads from an edge slot"""
    cout, cin = wgt.shape[:2]
    h = H // 2
    T = np.zeros((cin, h + 2, W + 2))                 # low rows -1 .. h, columns -1 .. W: zeros outside the image
    T[:, 1:h + 1, 1:W + 1] = _x_interp(low, W)
    src = np.arange(H, dtype=np.float64) * ((h - 1) / (H - 1))
    out = np.zeros((cout, H, W))

    def y_of(dy, r, x0, x1):
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
            mine = [{p: y_of(p[0], k0 + p[1], x0, x1) for p in owned(w)} for w in range(NCONS)]
            for w in range(NCONS):
                Y = dict(mine[w])
                for p in received(w) | edge_read(w):
                    (owner,) = [v for v in range(NCONS) if p in mine[v]]
                    Y[p] = mine[owner][p]
                for m in range(MW):
                    y = y0 + MW * w + m
                    z = np.zeros((cout, x1 - x0))
                    for dy in (-1, 0, 1):                         # fixed order: dy = -1, 0, +1, lower row first
                        yy = y + dy
                        if not 0 <= yy < H:
                            continue
                        r = 2 * w + ur_row(m, dy)
                        f = src[yy] - (k0 + r)
                        z += (1 - f) * Y[(dy, r)]
                        z += f * Y[(dy, r + 1)]
                    out[:, y, x0:x1] = z
    return out


@pytest.mark.parametrize("H,W", [(16, 32), (48, 80), (80, 48)])
def test_fold_over_the_balanced_plan_equals_conv_of_upsampled(H, W):
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(H * 1000 + W)
    low = rng.standard_normal((3, H // 2, W // 2))
    wgt = rng.standard_normal((2, 3, 3, 3))
    up = F.interpolate(torch.from_numpy(low)[None], scale_factor=2, mode="bilinear", align_corners=True)
    ref = F.conv2d(up, torch.from_numpy(wgt), padding=1)[0].numpy()
    got = fold(low, wgt, H, W)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
