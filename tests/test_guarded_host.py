"""The guard-band harness (tests/guarded.py) must be able to fail: each of its checks is driven here on CPU tensors with
a "kernel" that does the wrong thing on purpose (torch.as_strided on the arena; no kernel of the project runs).  And
the table of tests/test_gpu_guarded.py must cover include/unetpp.h: every launching symbol is declared by a row or sits
in the exclusion list with a reason."""
import numpy as np
import pytest
import torch

import guarded
import test_gpu_guarded as tg
from test_bindings_host import check_guard_coverage
from unet_amd import _lib


class Wrappers:
    """Stands in for PostProcessing: a wrapper that allocates as the real ones do and reaches the library through _call."""
    calls = []

    def _call(self, name, *args, stream_of=None):
        self.calls.append(name)

    def _workspace(self, n):
        return torch.empty(n, dtype=torch.uint8, device="cpu")

    def double(self, x, kernel):
        out = torch.empty_like(x)
        ws = self._workspace(64)
        counts = torch.zeros((3,), dtype=torch.int64, device="cpu")
        self._call("double", x, out, counts, ws, stream_of=x)
        kernel(x, out)
        return out


def run(kernel, x=None, **kw):
    x = np.arange(24, dtype=np.uint8).reshape(2, 12) if x is None else x

    def body(g):
        t = g.place(x, 1)
        with g.allocations(call_owner=Wrappers):
            return Wrappers().double(t, kernel)
    return guarded.two_fillings(torch, body, device="cpu", **kw), x


def honest(x, out):
    out.copy_(x * 2)


def test_an_honest_kernel_passes_and_every_buffer_is_in_an_arena():
    g = guarded.Guard(torch, "cpu", u8_out_offset=1)
    x = g.place(np.arange(24, dtype=np.float32).reshape(2, 12), 4)
    assert x.data_ptr() % 16 == 4 and x.is_contiguous() and np.array_equal(x.numpy(), np.arange(24, dtype=np.float32).reshape(2, 12))
    with g.allocations(call_owner=Wrappers):
        a = torch.empty((3, 5), dtype=torch.uint8, device="cpu")
        b = torch.zeros(7, dtype=torch.float64, device="cpu")
        c = torch.empty_like(x)
        ws = Wrappers()._workspace(33)
        host = torch.empty(4)                                  # no device given: not the harness's business
    assert a.data_ptr() % 16 == 1 and b.data_ptr() % 16 == 8 and c.data_ptr() % 16 == 4 and ws.data_ptr() % 16 == 0
    assert not b.any() and all(g.find(t) is not None for t in (x, a, b, c, ws)) and g.find(host) is None
    assert torch.empty is g._raw["empty"] and torch.zeros is g._raw["zeros"] and torch.empty_like is g._raw["empty_like"]
    assert all(a.lo >= guarded.MIN_GUARD and a.buf.numel() - a.hi >= guarded.MIN_GUARD for a in g.arenas)
    g.check()
    got, x = run(honest)
    assert np.array_equal(got[0][3], (x * 2).reshape(-1))


def test_a_write_one_element_past_the_end_is_caught():
    def kernel(x, out):
        honest(x, out)
        torch.as_strided(out, (out.numel() + 1,), (1,))[-1] = 7
    with pytest.raises(guarded.GuardError, match=r"back guard changed, payload-relative offsets 24 \.\. 24"):
        run(kernel)


def test_a_write_one_byte_before_the_start_is_caught():
    def kernel(x, out):
        honest(x, out)
        torch.as_strided(out, (1,), (1,), out.storage_offset() - 1)[0] ^= 0xFF
    with pytest.raises(guarded.GuardError, match=r"front guard changed, payload-relative offsets -1 \.\. -1"):
        run(kernel)


def test_a_tensor_from_outside_an_arena_is_caught_at_the_call():
    from unet_amd.postproc import PostProcessing
    g = guarded.Guard(torch, "cpu")
    with g.allocations(call_owner=Wrappers):
        inside = torch.empty((4,), dtype=torch.uint8, device="cpu")
        outside = inside.clone()
        Wrappers()._call("entry", inside, 3, None, inside[1:3])
        with pytest.raises(guarded.GuardError, match="entry, argument 2"):
            Wrappers()._call("entry", inside, 3, outside)
        g.exempt.add(("entry", 2))
        Wrappers()._call("entry", inside, 3, outside)
    with g.allocations():                                      # the real call layer: refused before the library is reached
        with pytest.raises(guarded.GuardError, match="unetpp_count_nonzero_u8, argument 0"):
            PostProcessing._call(object(), "unetpp_count_nonzero_u8", outside, 1, 2, 2, inside, stream_of=outside)
    assert PostProcessing._call.__name__ == "_call"            # and the hook is gone afterwards


def test_a_result_that_depends_on_a_guard_byte_is_caught_by_the_two_fillings():
    def kernel(x, out):
        honest(x, out)
        out[0, 0] += torch.as_strided(x, (x.numel() + 1,), (1,))[-1] & 1           # reads the byte behind its input
    with pytest.raises(guarded.GuardError, match="depends on bytes outside the tensors"):
        run(kernel)


def test_output_that_is_never_written_is_caught_by_the_two_fillings():
    def kernel(x, out):
        out[:, :-1].copy_(x[:, :-1] * 2)                       # forgets the last column
    with pytest.raises(guarded.GuardError, match="never written"):
        run(kernel)


# ---- the table of tests/test_gpu_guarded.py against the binding table ----------------------------------------------------------------
def test_every_launching_symbol_is_declared_by_a_row_or_excluded_with_a_reason():
    check_guard_coverage("unetpp.h")                           # the rule every family's module obeys
    declared = set().union(*(r.symbols for r in tg.ROWS)) | tg.NETWORK_SYMBOLS
    assert declared <= set(_lib.ABI), sorted(declared - set(_lib.ABI))          # and here a row reaches no other header's entries
    # what may be excluded: nothing that takes a stream (every launching entry ends in one) except the device-blob load,
    # which writes the engine's own weights, and only names of the kinds the reasons give
    kinds = ("_bytes", "_layout", "_create", "_destroy", "_last_error", "_version", "_status", "_load_", "_profile_", "_debug_")
    assert all(any(k in name for k in kinds) for name in tg.EXCLUDED), [n for n in tg.EXCLUDED if not any(k in n for k in kinds)]


def test_every_row_runs_at_the_placements_the_module_states():
    assert list(tg.PLACEMENTS)[:3] == ["P1", "P2", "P3"]
    assert tg.PLACEMENTS["P1"] == ((2, 32, 128), "aligned") and tg.PLACEMENTS["P2"] == ((2, 32, 128), "off") and tg.PLACEMENTS["P3"] == ((3, 33, 129), "off")
    assert tg.input_offset("aligned", 0, np.zeros(1, np.uint8), False) == 0 and tg.input_offset("off", 0, np.zeros(1, np.uint8), False) == 1
    assert tg.input_offset("off", 1, np.zeros(1, np.float32), False) == 4 and tg.input_offset("off", 1, np.zeros(1, np.float32), True) == 0
    assert tg.ROW_BY_NAME["nl_means"].shapes == {"P3b": (2, 129, 65)}
    assert tg.NET_SHAPES == [(1, 16, 16), (3, 16, 80), (2, 48, 80)]
    assert set(tg.NET_MODELS) == {("nested", "exact"), ("nested", "exact8"), ("nested", "fast"), ("simple", "exact")}
