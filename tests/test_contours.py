"""Host tests of unet_amd/contours.py (no GPU): the window-sum identity the device's contour areas rest on, checked against
the border-following restatement on every 4 x 5 mask and on random 12 x 12 masks; the restatement against the reference's
own functions (tests/golden/contours_scenes.npz, scripts/make_golden_contours.py); the exact circle; the overlay table; the
argument checks; what is particular to include/unetpp_contours.h."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from unet_amd import _lib
from unet_amd import components as cc
from unet_amd import contours as ct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "contours_scenes.npz")


# ---- the identity of DESIGN.md 5.22 ---------------------------------------------------------------------------------------------
def batch_window_area2(masks):
    """For bool masks [N,H,W], vectorised over N and written independently of contours.py: int64 [N, H W] holding, at the
    raster index of the first pixel of every 8-connected component of `inside`, the window sum of that component, and -1
    everywhere else."""
    n, h, w = masks.shape
    bg = np.ones((n, h + 2, w + 2), bool)
    bg[:, 1:-1, 1:-1] = ~masks
    out = np.zeros_like(bg)
    out[:, 0, :] = out[:, -1, :] = out[:, :, 0] = out[:, :, -1] = True
    while True:                                                     # flood the outside through 4-neighbours
        grown = out.copy()
        grown[:, 1:, :] |= out[:, :-1, :]; grown[:, :-1, :] |= out[:, 1:, :]
        grown[:, :, 1:] |= out[:, :, :-1]; grown[:, :, :-1] |= out[:, :, 1:]
        grown &= bg
        if (grown == out).all():
            break
        out = grown
    inside = ~out
    big = h * w + 1
    lab = np.full((n, h + 2, w + 2), big, np.int64)
    lab[:, 1:-1, 1:-1] = np.arange(1, h * w + 1).reshape(h, w)
    lab[~inside] = big
    while True:                                                     # every inside pixel takes the smallest index of its component
        m = lab.copy()
        for dy, dx in itertools.product((-1, 0, 1), repeat=2):
            src = lab[:, max(dy, 0):h + 2 + min(dy, 0), max(dx, 0):w + 2 + min(dx, 0)]
            dst = m[:, max(-dy, 0):h + 2 + min(-dy, 0), max(-dx, 0):w + 2 + min(-dx, 0)]
            np.minimum(dst, src, out=dst)
        m[~inside] = big
        if (m == lab).all():
            break
        lab = m
    lab[~inside] = 0
    q = np.stack((lab[:, :-1, :-1], lab[:, :-1, 1:], lab[:, 1:, :-1], lab[:, 1:, 1:]))
    cnt = (q > 0).sum(0)
    sums = np.bincount((np.arange(n)[:, None, None] * big + q.max(0)).reshape(-1), weights=np.maximum(cnt - 2, 0).reshape(-1),
                       minlength=n * big).astype(np.int64).reshape(n, big)
    roots = np.zeros((n, big), bool)
    core = lab[:, 1:-1, 1:-1].reshape(n, -1)
    roots[np.arange(n)[:, None], core] = True
    roots[:, 0] = False
    return np.where(roots, sums, -1)[:, 1:]


def traced_area2(masks):
    """The same table from the restatement: find_external_contours_np's tracer and Green's formula, mask by mask."""
    n, h, w = masks.shape
    pad = np.zeros((n, h + 2, w + 2), np.int8)
    pad[:, 1:-1, 1:-1] = masks
    out = np.full((n, h * w), -1, np.int64)
    for i, img in enumerate(pad.reshape(n, -1).tolist()):
        for pts in ct._trace_external(img, w + 2, h, w):
            out[i, pts[1] * w + pts[0]] = abs(ct._area2(pts))
    return out


def assert_identity(masks, what):
    got, want = batch_window_area2(masks), traced_area2(masks)
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, f"{what}: {bad.size} masks disagree, first:\n{masks[bad[0]].astype(int)}\nwindows {got[bad[0]]}\ncontours {want[bad[0]]}"


def test_window_identity_on_every_4x5_mask():
    """All 2^20 masks: one label of `inside` per external contour, at the contour's first pixel, and its window sum is twice
    the contourArea."""
    bits = np.arange(20)
    for lo in range(0, 1 << 20, 1 << 17):
        codes = np.arange(lo, lo + (1 << 17))
        assert_identity(((codes[:, None] >> bits) & 1).astype(bool).reshape(-1, 4, 5), f"codes {lo}..")


def test_window_identity_on_random_12x12_masks():
    r = np.random.default_rng(5)
    masks = np.concatenate([r.random((1000, 12, 12)) < p for p in (0.3, 0.5, 0.65, 0.8)])
    assert_identity(masks, "random 12x12")


def test_module_functions_agree_with_the_tracer_on_random_masks():
    """external_contour_areas_np (the form the device is compared with) against the contour list itself."""
    r = np.random.default_rng(6)
    for p in (0.35, 0.55, 0.75):
        for _ in range(40):
            m = (r.random((12, 17)) < p).astype(np.uint8) * 255
            labels, num, area2 = ct.external_contour_areas_np(m)
            contours = ct.find_external_contours_np(m)
            assert num == len(contours) + 1
            for l, c in enumerate(contours, 1):
                assert labels[c[0, 0, 1], c[0, 0, 0]] == l and area2[l] == 2 * ct.contour_area_np(c)
            on = np.zeros_like(m)
            for c in contours:                                      # every kept point lies on the outer border
                on[c[:, 0, 1], c[:, 0, 0]] = 1
            assert not (on & ~ct.outer_border_np(m)).any()
            want = 0.0 if not contours else 2 * ct.min_enclosing_circle_np(max(contours, key=ct.contour_area_np))[1]
            assert ct.measure_diameter_np(m) == want
            chosen, circle = ct.support_table_np(m)
            assert 2 * circle[1] == want and (chosen == 0) == (not contours)


def test_contours_of_small_shapes():
    z = np.zeros((5, 6), np.uint8)
    assert ct.find_external_contours_np(z) == [] and ct.measure_diameter_np(z) == 0.0
    one = z.copy(); one[2, 3] = 1
    (c,) = ct.find_external_contours_np(one)
    assert c.dtype == np.int32 and c.tolist() == [[[3, 2]]] and ct.contour_area_np(c) == 0.0 and ct.measure_diameter_np(one) == 0.0
    sq = z.copy(); sq[1:4, 1:5] = 1
    (c,) = ct.find_external_contours_np(sq)
    assert c[:, 0].tolist() == [[1, 1], [1, 3], [4, 3], [4, 1]] and ct.contour_area_np(c) == 6.0      # cv2's order: down the left side first
    assert ct.measure_diameter_np(sq) == np.sqrt(13.0)
    full = np.ones((3, 4), np.uint8)
    (c,) = ct.find_external_contours_np(full)
    assert ct.contour_area_np(c) == 6.0 and ct.outer_border_np(full).tolist() == [[1, 1, 1, 1], [1, 0, 0, 1], [1, 1, 1, 1]]
    ring = np.ones((7, 7), np.uint8); ring[1:6, 1:6] = 0; ring[3, 3] = 1            # the blob in the hole gives no contour
    (c,) = ct.find_external_contours_np(ring)
    assert ct.contour_area_np(c) == 36.0 and ct.outer_border_np(ring)[3, 3] == 0 and ct.inside_np(ring).all()


# ---- the circle -----------------------------------------------------------------------------------------------------------------
def test_circle_invariants_on_random_point_sets():
    r = np.random.default_rng(7)
    for trial in range(300):
        n = int(r.integers(1, 40))
        hi = int(r.choice([3, 12, 200, 4095]))
        pts = r.integers(0, hi + 1, (n, 2))
        sup = ct.support_set_np(pts.tolist())
        (cx, cy), rad = ct.min_enclosing_circle_np(pts)
        assert 1 <= len(sup) <= 3 and all(not ct._outside(sup, tuple(p)) for p in pts.tolist())          # exact containment
        d = np.hypot(pts[:, 0] - cx, pts[:, 1] - cy)
        assert (d <= rad * (1 + 1e-12) + 1e-300).all()
        distinct = len({tuple(p) for p in pts.tolist()})
        on = int((np.abs(d - rad) <= 1e-9 * max(rad, 1)).sum())
        assert (on >= 2) if distinct > 1 else (rad == 0.0)
        assert ct.min_enclosing_circle_np(pts[r.permutation(n)]) == ((cx, cy), rad)                       # order does not matter
        if n <= 12:                                                   # no smaller circle through 2 or 3 of the points holds them all
            best = rad
            P = [tuple(p) for p in pts.tolist()]
            for k in (2, 3):
                for s in itertools.combinations(sorted(set(P)), k):
                    try:
                        (x, y), q = ct.circle_from_points(s)
                    except ValueError:
                        continue
                    if q < best and (np.hypot(pts[:, 0] - x, pts[:, 1] - y) <= q * (1 + 1e-12)).all():
                        best = q
            assert best >= rad * (1 - 1e-12)


def test_circle_of_cocircular_points_does_not_depend_on_the_support_chosen():
    corners = [(0, 0), (40, 0), (0, 30), (40, 30)]
    want = ((20.0, 15.0), 25.0)
    assert ct.min_enclosing_circle_np(corners) == want
    for s in itertools.combinations(corners, 3):
        assert ct.circle_from_points(s) == want
    with pytest.raises(ValueError):
        ct.circle_from_points([(0, 0), (1, 1), (2, 2)])
    with pytest.raises(ValueError):
        ct.min_enclosing_circle_np([(0, 0), (4096, 0)])


# ---- paste and overlay ----------------------------------------------------------------------------------------------------------
def test_overlay_table_is_the_float64_expression():
    t = ct.overlay_table()
    assert t.shape == (3, 3, 256) and t.dtype == np.uint8
    for m, c, x in itertools.product(range(3), range(3), range(256)):
        px = np.array([[x, x, x]], np.uint8)
        assert t[m, c, x] == (px * 0.6 + np.array(ct.OVERLAY_COLOURS[m]) * 0.4).astype(np.uint8)[0, c]
    r = np.random.default_rng(8)
    frame = r.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    masks = [(r.random((9, 11)) < 0.5).astype(np.uint8) * 255 for _ in range(3)]
    chained = frame.copy()
    for m in range(3):
        for c in range(3):
            chained[..., c] = np.where(masks[m] > 0, t[m, c][chained[..., c]], chained[..., c])
    assert (ct.create_overlay_masks_np(frame, *masks) == chained).all()
    assert (ct.create_overlay_masks_np(frame, *[np.zeros((9, 11), np.uint8)] * 3) == frame).all()


def test_paste_clamps_like_the_reference():
    m = np.arange(1, 13, dtype=np.uint8).reshape(3, 4)
    out = ct.paste_roi_masks_np(m, (5, 4, 4, 3), (6, 7))                 # overhangs right and bottom
    assert out.shape == (6, 7) and (out[4:6, 5:7] == m[:2, :2]).all() and out.sum() == m[:2, :2].sum()
    out = ct.paste_roi_masks_np(m, (-2, -1, 6, 4), (6, 7))               # starts before the frame: pasted from (0, 0), as the reference does
    assert (out[:3, :4] == m).all() and out.sum() == m.sum()
    assert ct.paste_roi_masks_np(m[None], (9, 9, 4, 3), (6, 7)).sum() == 0


def test_argument_checks():
    with pytest.raises(ValueError):
        ct.find_external_contours_np(np.zeros((2, 3, 4), np.uint8))
    with pytest.raises(ValueError):
        ct.check_frame_shape(4096, 10)
    with pytest.raises(ValueError):
        ct.check_frame_shape(10, 5000)
    assert ct.check_frame_shape(4095, 4095) is None
    with pytest.raises(ValueError):
        ct.check_paste(3, 4, (9, 9, 4, 3), (6, 7))                       # the ROI misses the frame
    with pytest.raises(ValueError):
        ct.check_paste(3, 4, (0, 0, 4, 3), (6, 7, 1))
    with pytest.raises(ValueError):
        ct.check_max_components(1)
    # the in-circle determinant of the largest accepted coordinates fits int64 with room to spare
    m = ct.MAX_SIDE
    assert 6 * m * m * (2 * m * m) < 2 ** 62


# ---- the reference's own functions (scripts/make_golden_contours.py) -------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_golden_scenes_cover_the_cases(golden):
    names = [str(n) for n in golden["names"]]
    assert {"single_pixel", "diagonal_pair", "line", "disc", "ring_with_blob", "diagonal_touch", "all_edges", "zeros", "ones",
            "network_cable", "network_tape"} <= set(names)
    for n in names:
        m = golden[n + "/mask"]
        assert m.dtype == np.uint8 and 24 <= m.shape[0] <= 64 and 40 <= m.shape[1] <= 96
        a = golden[n + "/areas"]
        assert a.size < 2 or np.sort(a)[-1] > np.sort(a)[-2], f"{n}: two largest contours of equal area"


def test_restatement_against_the_reference(golden):
    for n in (str(v) for v in golden["names"]):
        m = golden[n + "/mask"]
        contours = ct.find_external_contours_np(m)
        assert [ct.contour_area_np(c) for c in contours] == golden[n + "/areas"].tolist(), n
        got, want = ct.measure_diameter_np(m), float(golden[n + "/diameter"])
        assert abs(got - want) <= 1e-12 * abs(want), (n, got, want)
        _, _, area2 = ct.external_contour_areas_np(m)
        assert (area2[1:] == 2 * golden[n + "/areas"]).all(), n
        assert 2 * ct.support_table_np(m)[1][1] == got, n
    assert int(golden["ring_with_blob/areas"].size) == 2              # the bar and the ring: the blob in the ring's hole gives none
    assert cc.components_np(golden["ring_with_blob/mask"], 8)[1].shape[0] - 1 == 3


def test_paste_and_overlay_against_the_reference(golden):
    for tag in ("paste_inside", "paste_overhang"):
        full = ct.paste_roi_masks_np(golden[tag + "/roi_mask"], golden[tag + "/roi"].tolist(), golden[tag + "/frame_hw"].tolist())
        assert (full == golden[tag + "/full"]).all(), tag
    got = ct.create_overlay_masks_np(golden["overlay/frame"], golden["overlay/cable"], golden["overlay/tape"], golden["overlay/burr"])
    assert (got == golden["overlay/out"]).all()


# ---- the header's entries (names, types, build inputs and guard coverage: tests/test_bindings_host.py) ------------------------------
def test_header_is_c99(tmp_path):
    cc_ = shutil.which("cc") or shutil.which("gcc")
    assert cc_, "no C compiler"
    src = tmp_path / "use.c"
    src.write_text('#include "unetpp_contours.h"\nint main(void) { int32_t t[UNETPP_CONTOURS_SUPPORT_COLUMNS] = {0}; (void)t; '
                   'return UNETPP_CONTOURS_MAX_SIDE - 4095; }\n')
    subprocess.run([cc_, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True, capture_output=True, text=True)


def test_entries_refuse_a_null_engine_and_bad_shapes():
    lib = _lib.load()
    assert lib.unetpp_contour_areas_u8(None, None, 1, 8, 8, -1, 16, None, None, None, None, None, None) == -1
    assert lib.unetpp_contour_circle(None, None, None, None, 1, 8, 8, 16, None, None, None) == -1
    assert lib.unetpp_paste_roi_u8(None, None, 1, 8, 8, 0, 0, 8, 8, 8, 8, None, None) == -1
    assert lib.unetpp_overlay_chain_u8(None, None, None, None, None, 1, 8, 8, None, None, None) == -1
    assert lib.unetpp_contours_workspace_bytes(1, 8, 8, 16) > 0
    assert lib.unetpp_contours_workspace_bytes(1, 4096, 8, 16) == 0 and lib.unetpp_contours_workspace_bytes(1, 8, 4096, 16) == 0
    assert lib.unetpp_contours_workspace_bytes(1, 8, 8, 1) == 0 and lib.unetpp_contours_workspace_bytes(0, 8, 8, 16) == 0
