"""CPU side of the morphology feature: the NumPy restatement (unet_amd/morphology.py) against known answers, scipy, a
direct per-offset loop and the fixtures made from the reference's own functions (scripts/make_golden_morph.py), and
the binding's bookkeeping.  The device side is tests/test_gpu_morphology.py.  Everything is boolean: exact equality."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import components as cc
from unet_amd import morphology as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows(e):
    return ["".join(str(int(v)) for v in r) for r in e]


def direct(x, e, anchor, dilate):
    """The definition, one offset at a time: outside pixels never contribute."""
    H, W = x.shape
    kh, kw = e.shape
    ax, ay = anchor
    acc = np.zeros((H, W), bool) if dilate else np.ones((H, W), bool)
    for i in range(kh):
        for j in range(kw):
            if not e[i, j]:
                continue
            dy, dx = i - ay, j - ax
            sh = np.full((H, W), not dilate, bool)
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y1 > y0 and x1 > x0:
                sh[y0:y1, x0:x1] = x[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            acc = (acc | sh) if dilate else (acc & sh)
    return acc


# ---- 1. structuring elements -----------------------------------------------------------------------------------------
def test_ellipse_known_answers():
    assert rows(mo.structuring_element("ellipse", 3)) == ["010", "111", "010"]
    assert rows(mo.structuring_element("ellipse", (5, 5))) == ["00100", "11111", "11111", "11111", "00100"]
    assert rows(mo.structuring_element("ellipse", 2)) == ["01", "11"]
    e8 = mo.structuring_element("ellipse", 8)
    assert e8.sum(1).tolist() == [1, 7, 7, 8, 8, 8, 7, 7]
    assert e8[0, 4] == 1 and all(int(np.argmax(e8[i])) == 1 for i in (1, 2, 6, 7))
    assert mo.structuring_element("ellipse", 15).sum(1).tolist() == [1, 9, 11, 13, 13, 15, 15, 15, 15, 15, 13, 13, 11, 9, 1]
    assert len({tuple(r) for r in mo.structuring_element("ellipse", 15)}) == 5
    assert len({tuple(r) for r in mo.structuring_element("ellipse", 21)}) == 7
    assert len({tuple(r) for r in mo.structuring_element("ellipse", 25)}) == 8


def test_rect_cross_one_by_one_and_non_square():
    assert mo.structuring_element("rect", (4, 2)).tolist() == [[1] * 4] * 2
    assert rows(mo.structuring_element("cross", (5, 3))) == ["00100", "11111", "00100"]
    for shape in mo.SHAPES:
        assert mo.structuring_element(shape, (1, 1)).tolist() == [[1]]
    e = mo.structuring_element("ellipse", (7, 3))
    assert e.shape == (3, 7) and e.dtype == np.uint8
    assert rows(e) == ["0001000", "1111111", "0001000"]
    assert rows(mo.structuring_element("ellipse", (3, 7))) == ["010", "111", "111", "111", "111", "111", "010"]
    with pytest.raises(ValueError, match="shape must be one of"):
        mo.structuring_element("diamond", 3)
    for shape, k in (("ellipse", 15), ("ellipse", 8), ("ellipse", 63), ("cross", 7), ("rect", (1, 9))):
        mo.check_element(mo.structuring_element(shape, k))          # all row-convex


# ---- 2. the primitives -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 5, 7, 15, 21])
def test_symmetric_elements_match_scipy(k):
    ndimage = pytest.importorskip("scipy.ndimage")
    r = np.random.default_rng(k)
    e = mo.structuring_element("ellipse", k)
    for density in (0.02, 0.5, 0.95):
        x = r.random((61, 83)) < density
        assert np.array_equal(mo.dilate_np(x, e), ndimage.binary_dilation(x, e, border_value=0))
        assert np.array_equal(mo.erode_np(x, e), ndimage.binary_erosion(x, e, border_value=1))
    c = mo.structuring_element("cross", 5)
    assert np.array_equal(mo.dilate_np(x, c, iterations=3), ndimage.binary_dilation(x, c, iterations=3))


def test_asymmetric_elements_match_the_definition():
    r = np.random.default_rng(8)
    custom = np.array([[0, 1, 1, 0, 0], [1, 1, 1, 1, 1], [0, 0, 0, 1, 0]], np.uint8)
    cases = [(mo.structuring_element("ellipse", 8), (4, 4)), (mo.structuring_element("ellipse", 2), (1, 1)), (custom, (4, 0)),
             (custom, (0, 2)), (mo.structuring_element("rect", (1, 9)), (0, 7))]
    for e, anchor in cases:
        for density in (0.03, 0.6, 0.97):
            x = r.random((40, 57)) < density
            default = anchor == (e.shape[1] // 2, e.shape[0] // 2)
            assert np.array_equal(mo.dilate_np(x, e, None if default else anchor), direct(x, e, anchor, True))
            assert np.array_equal(mo.erode_np(x, e, None if default else anchor), direct(x, e, anchor, False))
    # not reflected: a single pixel dilated by ELLIPSE (2,2) spreads to where the element, anchored at (1,1), sees it
    x = np.zeros((5, 5), bool); x[2, 2] = True
    assert np.argwhere(mo.dilate_np(x, mo.structuring_element("ellipse", 2))).tolist() == [[2, 2], [2, 3], [3, 2]]


def test_duality_fixed_points_ordering_and_iterations():
    r = np.random.default_rng(3)
    x = r.random((50, 70)) < 0.4
    for e in (mo.structuring_element("ellipse", 8), mo.structuring_element("ellipse", 5), mo.structuring_element("cross", 3)):
        assert np.array_equal(mo.erode_np(x, e), ~mo.dilate_np(~x, e))
        assert mo.erode_np(np.ones((9, 11), bool), e).all()              # outside pixels count as 1 for an erode
        assert not mo.dilate_np(np.zeros((9, 11), bool), e).any()
        assert np.array_equal(mo.dilate_np(x, e, iterations=2), mo.dilate_np(mo.dilate_np(x, e), e))
        assert np.array_equal(mo.erode_np(x, e, iterations=2), mo.erode_np(mo.erode_np(x, e), e))
    e = mo.structuring_element("ellipse", 5)
    for op, holds in (("open", lambda o: not (o & ~x).any()), ("close", lambda o: not (x & ~o).any())):
        el, steps, res = mo.program_single(op, e)
        o = mo.run_program_np(x.astype(np.uint8), None, el, steps, -1, -1, res, 1) != 0
        assert holds(o) and not np.array_equal(o, x)
    edge = np.zeros((20, 20), bool); edge[:, :6] = True                   # touches three edges: not eroded from them
    assert np.array_equal(mo.erode_np(edge, e), np.pad(np.ones((20, 4), bool), ((0, 0), (0, 16))))


# ---- 3. the fixtures from the reference's own functions ----------------------------------------------------------------
def test_restatement_reproduces_every_fixture_case():
    g = load_golden("morph_scenes")
    kinds = {}
    for tag, kind, H, W, seed, param, sha in (tuple(r) for r in g["cases"].tolist()):
        H, W, seed, param = int(H), int(W), int(seed), int(param)
        kinds[kind] = kinds.get(kind, 0) + 1
        unpack = lambda name: np.unpackbits(g[f"{tag}_{name}"])[:H * W].reshape(H, W)
        if kind == "holes":
            m = mo.make_hole_scene(H, W, seed, noise=0.0 if H < 100 else 0.02)
        else:
            m = cc.make_scene_mask(H, W, seed)
        assert hashlib.sha256(m.tobytes()).hexdigest() == sha, tag
        if kind == "ring_raw":
            got = mo.constrain_tape_to_ring_np(m, m, 2, 1)
            assert np.array_equal(got, unpack("out") * np.uint8(255)), tag
            assert got.any() and not np.array_equal(got != 0, m == 2)
        elif kind == "ring_largest":
            cable = cc.filter_components_np(m, 1, "largest", min_area=50)
            got = mo.constrain_tape_to_ring_np(m, cable, 2, -1)
            assert np.array_equal(got, unpack("out") * np.uint8(255)), tag
            assert got.any()
        elif kind == "cleanup":
            got = mo.cleanup_np(m, 2, param, 255)
            assert np.array_equal(got, unpack("out") * np.uint8(255)), tag
            assert int(((got != 0) != (m == 2)).sum()) >= 100
        elif kind == "postprocess":
            cable, tape = mo.postprocess_masks_np(m, 1, 2, W)
            assert np.array_equal(cable, unpack("cable") * np.uint8(255)), tag
            assert np.array_equal(tape, unpack("tape") * np.uint8(255)), tag
            assert bool(tape.any()) == (H == 512)                         # the 448 x 800 scenes fail the cable's gates
        else:
            n, area, holes = mo.tape_holes_np(m, 2, param)
            assert np.array_equal(holes, unpack("holes")), tag
            assert (n, area) == (int(g[tag + "_num_holes"]), int(g[tag + "_hole_area"])), tag
            assert len(cc.components_np(m, 8, 2)[1]) - 1 == int(g[tag + "_tape_components"])
            assert param != 3 or n >= 10
    assert kinds == {"ring_raw": 4, "ring_largest": 4, "cleanup": 8, "postprocess": 4, "holes": 6}


def test_make_hole_scene_leaves_make_scene_mask_alone():
    base = cc.make_scene_mask(96, 200, 2, 0.0)
    holes = mo.make_hole_scene(96, 200, 2, noise=0.0)
    changed = base != holes
    assert changed.any() and (base[changed] == 2).all() and (holes[changed] == 0).all()
    assert np.array_equal(base, cc.make_scene_mask(96, 200, 2, 0.0))


# ---- 4. binding and argument checks ------------------------------------------------------------------------------------
def test_binding_lists_the_morphology_symbols():
    from unet_amd import _lib
    assert {"unetpp_morphology", "unetpp_morphology_layout"} <= set(_lib.ABI_SYMBOLS)
    assert "morphology.h" in _lib.HEADERS
    header = open(os.path.join(ROOT, "include", "unetpp.h")).read()
    enum = {n.lower(): int(v) for n, v in re.findall(r"UNETPP_MORPH_([A-Z]+) = (\d+)", header)}
    assert enum == _lib.MORPH_OPS == mo.OPS and len(enum) == 6
    assert [n for n, _ in _lib.MorphElement._fields_] == ["kw", "kh", "ax", "ay", "host_data"]
    assert [n for n, _ in _lib.MorphStep._fields_] == ["op", "dst", "a", "b", "element", "iterations"]
    assert mo.MAX_K == 63


def test_layout_query_and_error_codes_without_a_device():
    """unetpp_morphology_layout is host code: the program checks of the C ABI run here."""
    from unet_amd import _lib
    lib = ctypes.CDLL(_lib.build())
    lib.unetpp_morphology_layout.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(_lib.MorphElement), ctypes.c_int,
                                                                  ctypes.POINTER(_lib.MorphStep), ctypes.c_int,
                                                                  ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]

    def layout(h, w, element, steps, batch=16, anchor=(-1, -1)):
        e = np.ascontiguousarray(element, np.uint8)
        el = (_lib.MorphElement * 1)(_lib.MorphElement(e.shape[1], e.shape[0], anchor[0], anchor[1], e.ctypes.data))
        st = (_lib.MorphStep * len(steps))(*[_lib.MorphStep(*s) for s in steps])
        band, cols = ctypes.c_int(-1), ctypes.c_int(-1)
        rc = lib.unetpp_morphology_layout(batch, h, w, el, 1, st, len(steps), ctypes.byref(band), ctypes.byref(cols))
        return rc, band.value, cols.value

    e5, e63 = mo.structuring_element("ellipse", 5), mo.structuring_element("ellipse", 63)
    close = lambda n: [(0, 2, 0, 0, 0, n), (1, 2, 2, 0, 0, n)]
    rc, band, cols = layout(512, 512, e5, close(1))
    assert rc == 0 and 1 <= band <= 512 and cols == 512
    rc, band, cols = layout(512, 4096, e63, close(1))                      # the halo does not fit full-width rows: tiles
    assert rc == 0 and band >= 1 and cols % 64 == 0 and cols < 4096
    assert layout(300, 4096, e5, close(2) + [(0, 2, 2, 0, 0, 1)])[0] == 0
    assert layout(1, 1, e63, close(1))[0] == 0
    assert layout(512, 512, e63, close(1) + [(0, 2, 2, 0, 0, 1)])[0] == -2         # reach 3 * 62 > 126
    assert layout(512, 512, np.ones((3, 64), np.uint8), close(1))[0] == -2          # too large
    assert layout(512, 512, np.array([[1, 0, 1]], np.uint8), close(1))[0] == -2     # not row-convex
    assert layout(512, 512, np.zeros((3, 3), np.uint8), close(1))[0] == -1          # empty
    assert layout(512, 512, e5, [(0, 2, 0, 0, 0, 0)])[0] == -1                      # iterations < 1
    assert layout(512, 512, e5, [(0, 2, 3, 0, 0, 1)])[0] == -1                      # scratch plane read before written
    assert layout(512, 512, e5, [(0, 2, 0, 0, 1, 1)])[0] == -1                      # element index
    assert layout(512, 512, e5, [(6, 2, 0, 0, 0, 1)])[0] == -1                      # op
    assert layout(512, 512, e5, [(0, 4, 0, 0, 0, 1)])[0] == -1                      # plane index
    assert layout(512, 512, e5, close(1), anchor=(5, 0))[0] == -1                   # anchor outside
    assert layout(0, 512, e5, close(1))[0] == -1


def test_methods_check_their_arguments_without_a_device():
    from unet_amd.nested_unet import NestedUNet, SimpleUNet
    for model in (NestedUNet(3), SimpleUNet(3)):
        with pytest.raises(RuntimeError, match="uint8 CUDA tensor"):
            model.morphology(np.zeros((1, 4, 4), np.uint8), ksize=8)                 # even-sized is fine, a host array is not
        with pytest.raises(ValueError, match="at most 63x63"):
            model.morphology(None, ksize=64, shape="rect")
        with pytest.raises(ValueError, match="not row-convex"):
            model.morphology(None, element=np.array([[1, 0, 1]], np.uint8))
        with pytest.raises(ValueError, match="empty"):
            model.morphology(None, element=np.zeros((3, 3), np.uint8))
        with pytest.raises(ValueError, match="op must be one of"):
            model.morphology(None, op="gradient")
        with pytest.raises(ValueError, match="iterations must be at least 1"):
            model.morphology(None, iterations=0)
        with pytest.raises(ValueError, match="out_value"):
            model.morphology(None, out_value=256)
        with pytest.raises(ValueError, match="anchor"):
            model.morphology(None, ksize=3, anchor=(3, 1))
        with pytest.raises(ValueError, match="op must be one of"):
            model.morphology_program(None, -1, [("xor", 2, 0, 1)], [])
        with pytest.raises(ValueError, match="before any step has written it"):
            model.morphology_program(None, -1, [("and", 2, 0, 3)], [])
        with pytest.raises(ValueError, match="result_plane"):
            model.morphology_program(None, -1, [("copy", 2, 0)], [], result_plane=3)
        with pytest.raises(ValueError, match="at most 8 steps"):
            model.morphology_program(None, -1, [("copy", 2, 0)] * 9, [])
        with pytest.raises(ValueError, match="reach"):
            model.morphology(None, ksize=63, iterations=2, op="close")
        with pytest.raises(RuntimeError, match="uint8 CUDA tensor"):
            model.tape_holes(np.zeros((1, 4, 4), np.uint8))
