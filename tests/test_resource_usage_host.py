"""Register budget of the wave-specialised kernels, from the compiler's own kernel-resource-usage remarks
(scripts/resource_usage.py; no GPU, about a minute of hipcc).  A scalar the register allocator cannot place goes into a
vector lane and comes back through v_readlane in front of its use -- in the producers that is in front of a DMA instruction,
on the SIMD the consumers' MFMA stream runs on.  Every instantiation the flagship runs stays at zero."""
import importlib.util
import os
import shutil

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")

WS = "conv3x3_ws_kernel<2, {}, {}, {}, {}, {}, {}, false, false>"
# (POOL, HEAD, UPF, C0F, NW, MW) of the `exact` launches of the 3-class 512 x 512 batch-16 forward
FLAGSHIP = [
    ("false", "false", "false", "false", 2, 2),      # Cout >= 64 convs: the dominant kernel
    ("true", "false", "false", "false", 2, 2),       # encoder conv2 + pool, levels 1-3
    ("false", "false", "true", "false", 2, 2),       # conv1_x.conv1 + upsample
    ("false", "false", "true", "false", 1, 4),       # conv0_x.conv1 + upsample
    ("false", "true", "false", "false", 1, 4),       # conv0_4.conv2 + head + argmax
    ("true", "false", "false", "true", 1, 4),        # fused first block
    ("false", "false", "false", "false", 1, 4),      # 32-channel convs
    ("true", "false", "false", "false", 1, 4),
]


@pytest.fixture(scope="module")
def ru():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "scripts", "resource_usage.py"))
    ru = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ru)
    return ru


@pytest.fixture(scope="module")
def kernels(ru):
    table = ru.parse_remarks(ru.compile_remarks())
    print(ru.table(table, ["conv3x3_ws", "tapmm_ws_kernel"]))
    return table


@pytest.mark.parametrize("targs", FLAGSHIP, ids=lambda t: ",".join(str(v)[0].upper() if isinstance(v, str) else str(v) for v in t))
def test_flagship_conv_kernels_spill_nothing(targs, kernels):
    k = kernels[WS.format(*targs)]
    assert k["sgpr_spill"] == 0, k
    assert k["vgpr_spill"] == 0 and k["scratch"] == 0, k
    assert k["occupancy"] == 2, k


@pytest.mark.parametrize("name", ["tapmm_ws_kernel<false>", "tapmm_ws_kernel<true>"])
def test_tapmm_stays_without_spills(name, kernels):
    k = kernels[name]
    assert k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0 and k["scratch"] == 0 and k["occupancy"] == 2, k


def test_no_wave_specialised_kernel_uses_scratch_or_loses_occupancy(kernels):
    """exact8, SimpleUNet's two-source and the split-K instantiations share the source: none may pay for the change"""
    ws = {n: k for n, k in kernels.items() if n.startswith("conv3x3_ws")}
    assert len(ws) >= 18
    for n, k in ws.items():
        assert k["vgpr_spill"] == 0 and k["scratch"] == 0 and k["occupancy"] == 2, (n, k)


def test_measurement_build_compiles_the_same_kernels(ru, kernels):
    """-DUNETPP_WS_DBG=1 (csrc/ws_dbg_dev.h, ws_dbg_host.h; scripts/ws_ablate.sh) is built by hand and rarely: it must go on
    compiling, into the kernels of the product build.  Its registers are its own business (the stamps cost some)."""
    dbg = ru.parse_remarks(ru.compile_remarks(defines=["UNETPP_WS_DBG=1"]))      # raises if the compile fails
    assert set(dbg) == set(kernels)
