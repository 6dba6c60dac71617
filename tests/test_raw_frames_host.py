"""Raw camera frames without a GPU: the NumPy forms of unet_amd/raw_frames.py against an independent second form, OpenCV's
documented pattern names and the reference's own _to_bgr (tests/golden/raw_scenes.npz, README_raw.txt), and what is particular to
include/unetpp_raw.h: its enum, its C99 form, the null-engine codes and the guard rows the family requires."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import _lib
from unet_amd import raw_frames as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unetpp_raw.h")
BAYER = ("BG", "GB", "RG", "GR")


@pytest.fixture(scope="module")
def golden():
    g = load_golden("raw_scenes")
    return {k: g[k] for k in g.files}


def scalar_demosaic(raw, pattern):
    """The issue's wording pixel by pixel, interior then the clamp rule: no array expression shared with demosaic_np."""
    h, w = raw.shape
    v = raw.astype(int)
    (ry, rx) = rf.RED_SITE[pattern]
    inner = np.zeros((h, w, 3), np.uint8)
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            cross = (v[y - 1, x] + v[y + 1, x] + v[y, x - 1] + v[y, x + 1] + 2) >> 2
            diag = (v[y - 1, x - 1] + v[y - 1, x + 1] + v[y + 1, x - 1] + v[y + 1, x + 1] + 2) >> 2
            hor, ver = (v[y, x - 1] + v[y, x + 1] + 1) >> 1, (v[y - 1, x] + v[y + 1, x] + 1) >> 1
            if (y & 1, x & 1) == (ry, rx):
                b, g, r = diag, cross, v[y, x]
            elif (y & 1, x & 1) == (1 - ry, 1 - rx):
                b, g, r = v[y, x], cross, diag
            elif (y & 1) == ry:                                   # a green site in a row of red sites: red lies left and right
                b, g, r = ver, v[y, x], hor
            else:
                b, g, r = hor, v[y, x], ver
            inner[y, x] = (b, g, r)
    out = np.zeros_like(inner)
    for y in range(h):
        for x in range(w):
            out[y, x] = inner[min(max(y, 1), h - 2), min(max(x, 1), w - 2)]
    return out


# ---- 1. the arithmetic ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 3), (4, 5), (5, 4), (7, 9), (33, 17)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("pattern", BAYER)
def test_interior_equals_the_correlation_form(pattern, shape):
    raw = rf.make_raw(1, shape[0], shape[1], 31 * shape[0] + shape[1])[0]
    got = rf.demosaic_np(raw, pattern)
    assert got.dtype == np.uint8 and got.shape == shape + (3,)
    assert np.array_equal(got[1:-1, 1:-1], rf.correlation_form_np(raw, pattern))
    r = np.random.default_rng(shape[0])                               # and on bytes with no structure at all
    noise = r.integers(0, 256, shape, dtype=np.uint8)
    assert np.array_equal(rf.demosaic_np(noise, pattern)[1:-1, 1:-1], rf.correlation_form_np(noise, pattern))


@pytest.mark.parametrize("pattern", BAYER)
def test_border_is_the_clamp_rule_and_the_smallest_frames(pattern):
    for h, w in ((3, 3), (3, 8), (8, 3), (6, 7), (9, 12)):
        raw = np.random.default_rng(h * w).integers(0, 256, (h, w), dtype=np.uint8)
        got = rf.demosaic_np(raw, pattern)
        assert np.array_equal(got, scalar_demosaic(raw, pattern)), (h, w)
        ys, xs = np.clip(np.arange(h), 1, h - 2), np.clip(np.arange(w), 1, w - 2)
        assert np.array_equal(got, got[ys[:, None], xs[None, :]])
    for bad in ((2, 8), (8, 2), (1, 1)):
        with pytest.raises(ValueError, match="needs H, W >= 3"):
            rf.demosaic_np(np.zeros(bad, np.uint8), pattern)
    batch = rf.make_raw(3, 6, 7, 0)
    assert np.array_equal(rf.demosaic_np(batch, pattern), np.stack([rf.demosaic_np(f, pattern) for f in batch]))


def test_pattern_names_follow_opencv_documentation():
    """'The two letters indicate the particular pattern type: the components in the second row, second and third columns.'"""
    for pattern in BAYER:
        named = []
        for y, x in ((1, 1), (1, 2)):
            raw = np.zeros((4, 4), np.uint8)
            raw[y, x] = 200
            bgr = rf.demosaic_np(raw, pattern)[y, x]
            assert sorted(bgr.tolist()) == [0, 0, 200]                # the pixel measures exactly one component
            named.append("BGR"[int(np.argmax(bgr))])
        assert "".join(named) == pattern
    assert rf.RED_SITE == {"BG": (0, 0), "GB": (0, 1), "RG": (1, 1), "GR": (1, 0)} and rf.PATTERNS == {"BG": 0, "GB": 1, "RG": 2, "GR": 3, "MONO": 4}


def test_mono_and_gray():
    raw = rf.make_raw(2, 5, 6, 1)
    bgr = rf.demosaic_np(raw, "MONO")
    assert bgr.shape == (2, 5, 6, 3) and all(np.array_equal(bgr[..., c], raw) for c in range(3))
    assert np.array_equal(rf.gray_np(raw, "MONO"), raw)               # 3735 + 19235 + 9798 = 2^15
    assert rf.demosaic_np(np.zeros((1, 2), np.uint8), "MONO").shape == (1, 2, 3)
    from unet_amd import edges as ed
    assert np.array_equal(rf.gray_np(raw, "GR"), ed.bgr_to_gray_np(rf.demosaic_np(raw, "GR")))
    with pytest.raises(ValueError, match="pattern must be one of"):
        rf.demosaic_np(raw, "RGGB")
    with pytest.raises(ValueError, match="raw must be uint8"):
        rf.demosaic_np(raw.astype(np.int32), "RG")


# ---- 2. the reference's _to_bgr -------------------------------------------------------------------------------------------------------
def test_to_bgr_np_equals_the_reference_for_every_name(golden):
    cases = golden["cases"]
    assert sorted({c[1] for c in cases}) == sorted(rf.FIXTURE_FORMATS) and len(cases) == len(rf.FIXTURE_FORMATS) * len(rf.FIXTURE_SHAPES)
    from unet_amd.simple_loops import sha
    for tag, fmt, h, w, seed, code, in_sha, out_sha in cases:
        h, w = int(h), int(w)
        buffer = rf.make_raw(1, h, w, int(seed))[0].reshape(-1)
        assert sha(buffer) == in_sha, tag
        got = rf.to_bgr_np(buffer, fmt, w, h)
        assert np.array_equal(got, golden[tag + "_out"]) and sha(got) == out_sha, tag
        assert int(code) == {"RG": 48, "BG": 46, "MONO": 8}[rf.pattern_of(fmt)], tag
    assert [rf.pattern_of(n) for n in ("BayerRG8", "BayerRG12", "BayerBG8", "Mono8", "BayerGR8", "BayerGB8", "whatever")] == \
           ["RG", "RG", "BG", "MONO", "MONO", "MONO", "MONO"]
    with pytest.raises(ValueError):
        rf.to_bgr_np(np.zeros(10, np.uint8), "BayerRG8", 4, 3)        # the reshape itself refuses


# ---- 3. the fused form -----------------------------------------------------------------------------------------------------------------
def test_raw_resize_takes_the_phase_from_the_frame():
    from unet_amd import tiling as tl
    raw = rf.make_raw(1, 37, 53, 9)[0]
    for pattern in BAYER:
        for roi in ((5, 3, 40, 31), (4, 3, 40, 31), (5, 2, 40, 31)):
            x0, y0, cw, ch = roi
            got = rf.raw_resize_np(raw, pattern, roi, (16, 24))
            assert got.shape == (16, 24, 3)
            assert np.array_equal(got, tl.resize_linear_u8_np(rf.demosaic_np(raw, pattern)[y0:y0 + ch, x0:x0 + cw], (24, 16)))
            from_crop = rf.raw_resize_np(np.ascontiguousarray(raw[y0:y0 + ch, x0:x0 + cw]), pattern, None, (16, 24))
            assert not np.array_equal(got, from_crop), (pattern, roi)      # an odd origin shifts the crop's own phase
    even = rf.raw_resize_np(raw, "RG", (4, 2, 20, 20), (20, 20))[1:-1, 1:-1]   # an even origin and no scaling: only the border differs
    assert np.array_equal(even, rf.demosaic_np(np.ascontiguousarray(raw[2:22, 4:24]), "RG")[1:-1, 1:-1])
    assert np.array_equal(rf.raw_resize_np(raw, "GB", None, (37, 53)), rf.demosaic_np(raw, "GB"))
    batch = rf.make_raw(2, 9, 11, 2)
    assert np.array_equal(rf.raw_resize_np(batch, "GR", (1, 3, 9, 5), (32, 16)), np.stack([rf.raw_resize_np(f, "GR", (1, 3, 9, 5), (32, 16)) for f in batch]))
    for bad in ((0, 0, 54, 37), (-1, 0, 4, 4), (0, 0, 0, 4), (50, 0, 4, 4)):
        with pytest.raises(ValueError, match="does not lie inside"):
            rf.raw_resize_np(raw, "RG", bad, (8, 8))


# ---- 4. the header's entries (names, types, build inputs and guard coverage: tests/test_bindings_host.py) -------------------------------
def test_raw_patterns_are_the_headers_enum():
    with open(HEADER) as f:
        text = f.read()
    for name, value in _lib.RAW_PATTERNS.items():
        assert re.search(r"\bUNETPP_RAW_%s = %d\b" % (name, value), text), name


def test_header_is_c99(tmp_path):
    cc_ = shutil.which("cc") or shutil.which("gcc")
    assert cc_, "no C compiler"
    src = tmp_path / "use.c"
    src.write_text('#include "unetpp_raw.h"\nint main(void) { return UNETPP_RAW_BG + (UNETPP_RAW_MONO != 4) + (UNETPP_RAW_GR != 3); }\n')
    subprocess.run([cc_, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True, capture_output=True, text=True)


def test_entries_refuse_a_null_engine():
    lib = _lib.load()
    assert lib.unetpp_raw_to_bgr_u8(None, None, 8, 64, 1, 8, 8, 0, None, None, None) == -1
    assert lib.unetpp_raw_resize_u8(None, None, 8, 64, 1, 8, 8, 0, 0, 0, 8, 8, None, 4, 4, None) == -1


def test_guard_rows_the_family_requires():
    import test_gpu_guarded_raw as tgr
    names = [r.name for r in tgr.ROWS_RAW]
    assert any(n.startswith("process_raw_frames") for n in names)
    assert {"to_bgr[BayerBG8, both]", "to_gray[RG]", "to_bgr[RG]"} <= set(names)          # BGR, grey, both
