"""Launch planning restated on the host (no device): the tile-number stepping of the persistent conv kernels, the split-K rule
of launch_ws_k and the parsing of UNETPP_PLAN_CUS.  The restatements pin the ALGORITHMS (csrc/conv3x3_ws.h decode_first /
decode_next / tile_step, csrc/unetpp_abi.hip launch_ws_k); tests/test_gpu_plan_sweep.py pins the kernels that run them."""
import ctypes

import numpy as np
import pytest


# ---- the walk: tile number -> (split share, channel tile, column, row, image) ---------------------------------------------------

def gdec(G, ks, nct, tx, ty):
    """launch_ws_k: the grid size in the tile-number radix, written down digit by digit for the kernel"""
    t = G
    d = [t % ks]; t //= ks
    d.append(t % nct); t //= nct
    d.append(t % tx); t //= tx
    d.append(t % ty)
    d.append(t // ty)
    return d


def decode_first(t, ks, nct, tx, ty):
    """a workgroup's first tile: four divisions (np arrays or ints)"""
    u, dks = t // ks, t % ks
    u, dct = u // nct, u % nct
    u, dtx = u // tx, u % tx
    return [dks, dct, dtx, u % ty, u // ty]


def decode_next(cur, g, ks, nct, tx, ty):
    """every later tile: add the grid size's digits, carries through the radix (the image digit has no bound of its own)"""
    dks, dct, dtx, dty, dn = cur
    dks = dks + g[0]
    carry = dks >= ks; dks = dks - np.where(carry, ks, 0)
    dct = dct + g[1] + carry
    carry = dct >= nct; dct = dct - np.where(carry, nct, 0)
    dtx = dtx + g[2] + carry
    carry = dtx >= tx; dtx = dtx - np.where(carry, tx, 0)
    dty = dty + g[3] + carry
    carry = dty >= ty; dty = dty - np.where(carry, ty, 0)
    return [dks, dct, dtx, dty, dn + g[4] + carry]


def head_step(g, nct, tx, ty):
    """the HEAD variant's tile_step(): the step put together again from gdec at every tile (no split-K with a head)"""
    return ((g[4] * ty + g[3]) * tx + g[2]) * nct + g[1]


def xcd_slot(b, G):
    return (b % 8) * (G // 8) + b // 8 if G % 8 == 0 else b


def radices():
    rng = np.random.default_rng(20261020)
    out = [(1, 1, 3, 3, 3), (1, 2, 2, 2, 3), (4, 8, 1, 1, 2), (16, 8, 40, 40, 32), (1, 1, 1, 1, 1), (1, 1, 16, 32, 16), (8, 2, 1, 2, 1)]
    for _ in range(24):
        out.append((int(rng.integers(1, 17)), int(rng.integers(1, 9)), int(rng.integers(1, 41)), int(rng.integers(1, 41)),
                    int(rng.integers(1, 33))))
    return out


def test_stepping_by_the_grid_size_visits_slot_plus_k_grids():
    """For random radices (ks <= 16, nct <= 8, tiles_x, tiles_y <= 40, images <= 32) and every grid size G from 1 to 300: one
    decode_next from the digits of any tile t gives the digits of t + G, checked against divmod.  decode_first IS divmod, so by
    induction a workgroup that starts at its slot visits exactly slot + k G.  Up to 6144 tiles every t is checked, above that the
    first and last 2048 and 2048 random ones (carries do not depend on where in the range a tile lies, only on its digits).
    This pins the algorithm; tests/test_gpu_plan_sweep.py pins the kernel."""
    rng = np.random.default_rng(7)
    for ks, nct, tx, ty, n in radices():
        total = ks * nct * tx * ty * n
        ts = np.arange(total) if total <= 6144 else np.unique(np.concatenate(
            [np.arange(2048), np.arange(total - 2048, total), rng.integers(0, total, 2048)]))
        first = decode_first(ts, ks, nct, tx, ty)
        assert all((d >= 0).all() for d in first) and (first[4] < n).all()
        for G in range(1, 301):
            grid = min(G, total)                      # launch_ws_k: min(tiles, CUs)
            g = gdec(grid, ks, nct, tx, ty)
            assert g[0] < ks and g[1] < nct and g[2] < tx and g[3] < ty
            if ks == 1:
                assert head_step(g, nct, tx, ty) == grid
            sel = ts + grid < total
            got = decode_next([d[sel] for d in first], g, ks, nct, tx, ty)
            want = decode_first(ts[sel] + grid, ks, nct, tx, ty)
            for a, b in zip(got, want):
                assert np.array_equal(a, b), (ks, nct, tx, ty, n, G)


@pytest.mark.parametrize("radix,G", [((1, 1, 3, 3, 3), 5), ((1, 2, 2, 2, 3), 7), ((4, 2, 1, 1, 2), 3), ((1, 8, 1, 1, 3), 16),
                                     ((2, 1, 5, 3, 2), 24), ((1, 1, 3, 3, 3), 27), ((3, 2, 7, 5, 4), 256)])
def test_a_whole_launch_walked_tile_by_tile(radix, G):
    """The loop as the kernel runs it: every workgroup starts at its (XCD-permuted) slot, steps while tile < total; together the
    workgroups visit every tile exactly once, each with the digits divmod gives."""
    ks, nct, tx, ty, n = radix
    total = ks * nct * tx * ty * n
    grid = min(G, total)
    g = gdec(grid, ks, nct, tx, ty)
    seen = []
    for b in range(grid):
        tile = xcd_slot(b, grid)
        cur = decode_first(tile, ks, nct, tx, ty)
        while tile < total:
            assert [int(v) for v in cur] == decode_first(tile, ks, nct, tx, ty)
            seen.append(tile)
            tile += grid
            cur = decode_next(cur, g, ks, nct, tx, ty)
    assert sorted(seen) == list(range(total))


def test_xcd_slot_map_is_a_permutation():
    for G in range(8, 1025, 8):
        assert sorted(xcd_slot(b, G) for b in range(G)) == list(range(G))
    # workgroups b, b + 8, ... (one XCD under round-robin dispatch) get a contiguous run of slots
    assert [xcd_slot(b, 32) for b in range(0, 32, 8)] == [0, 1, 2, 3]


# ---- the split-K rule ----------------------------------------------------------------------------------------------------------

def ksplit_loop(tiles, nchunks, n, pair9, kmax=16, minc=4, gate=4):
    """launch_ws_k, as written"""
    ks = 1
    if kmax > 1 and tiles * gate <= n:
        d = 2
        while d <= kmax and tiles * d <= n and nchunks // d >= minc:
            if nchunks % d == 0 and not (pair9 and (nchunks // d) % 2):
                ks = d
            d += 1
    return ks


def ksplit_rule(tiles, nchunks, n, pair9):
    """... and as DESIGN.md 5.5 words it: the largest divisor d <= 16 of the chunk count with tiles d <= n and nchunks / d >= 4
    (whole chunk pairs under pair9), for launches with tiles 4 <= n; otherwise no split"""
    if tiles * 4 > n:
        return 1
    ok = [d for d in range(2, 17) if nchunks % d == 0 and tiles * d <= n and nchunks // d >= 4 and not (pair9 and (nchunks // d) % 2)]
    return max(ok, default=1)


def test_split_k_rule_never_plans_more_workgroups_than_cus():
    """The partial sums and arrival counters hold one record per planned CU (unetpp_create): a split launch must have
    tiles * ksplit <= n workgroups for every planned CU count n, 1 to 1024."""
    splits = set()
    for n in range(1, 1025):
        for tiles in (1, 2, 3, 4, 5, 6, 8, 12, 15, 16, 24, 27, 32, 54, 64, 100, 128, 255, 256):
            if tiles * 4 > n:
                assert ksplit_loop(tiles, 32, n, False) == 1
                continue
            for nchunks in (1, 2, 3, 4, 6, 8, 9, 12, 16, 18, 24, 32, 36, 48, 64, 96):
                for pair9 in (False, True):
                    ks = ksplit_loop(tiles, nchunks, n, pair9)
                    assert ks == ksplit_rule(tiles, nchunks, n, pair9), (tiles, nchunks, n, pair9)
                    assert tiles * ks <= n and nchunks % ks == 0 and (ks == 1 or nchunks // ks >= 4), (tiles, nchunks, n, ks)
                    assert not (pair9 and ks > 1 and (nchunks // ks) % 2)
                    splits.add(ks)
    assert splits == {1, 2, 3, 4, 6, 8, 9, 12, 16}
    # the plans tests/test_gpu_plan_sweep.py asks for at 2 x 96 x 160: conv4_0 (2 images x 8 channel tiles, 16 + 32 chunks)
    assert [ksplit_loop(16, 32, n, False) for n in (64, 128, 256)] == [4, 8, 8] and ksplit_loop(16, 16, 64, False) == 4


# ---- UNETPP_PLAN_CUS -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", ["", "abc", "0", "-3", "12x", "1.5", " ", "0x10", "99999999999999999999"])
def test_plan_cus_override_refuses_malformed_values_before_the_device_is_queried(value, monkeypatch):
    """A non-number or a value below 1: UNETPP_E_INVALID and a message that names the variable -- with or without a device."""
    from unet_amd import _lib
    lib = _lib.load()
    monkeypatch.setenv("UNETPP_PLAN_CUS", value)
    cfg = _lib.Config(3, 3, 1, 32, 32, 0, 0, 0, 1, 0)
    h = ctypes.c_void_p()
    rc = lib.unetpp_create(ctypes.byref(cfg), ctypes.byref(h))
    assert rc == -1 and not h.value                               # UNETPP_E_INVALID
    msg = lib.unetpp_last_error(None).decode()
    assert "UNETPP_PLAN_CUS" in msg and repr(value)[1:-1] in msg, msg


def test_plan_cus_override_accepts_a_whole_number():
    """A well-formed value passes the parser: what follows is the device query (without a device: its error, not the parser's)."""
    import os
    from unet_amd import _lib
    lib = _lib.load()
    cfg = _lib.Config(3, 3, 1, 32, 32, 0, 0, 0, 1, 0)
    h = ctypes.c_void_p()
    old = os.environ.get("UNETPP_PLAN_CUS")
    os.environ["UNETPP_PLAN_CUS"] = "1"
    try:
        rc = lib.unetpp_create(ctypes.byref(cfg), ctypes.byref(h))
    finally:
        os.environ.pop("UNETPP_PLAN_CUS")
        if old is not None:
            os.environ["UNETPP_PLAN_CUS"] = old
    if rc == 0:
        lib.unetpp_destroy(h)
    else:
        assert "UNETPP_PLAN_CUS" not in lib.unetpp_last_error(None).decode()
