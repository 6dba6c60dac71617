"""ctypes binding of include/optim/unetpp_optim.h and the in-tree build of libunetpp_optim_hip.so, the optimiser step's own
library (unet-_amd/csrc_optim/).  The conventions are those of _lib.py: one table from symbol to ctypes types, a source hash
baked into the binary, a build that writes aside and renames, and no CPU fallback: a missing or stale library that cannot be
rebuilt is an error."""
from __future__ import annotations

import ctypes
import hashlib
import os
import subprocess

from . import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libunetpp_optim_hip.so")
CSRC = os.path.join(_HERE, "csrc_optim")
SOURCES = ["unetpp_optim.hip"]
HEADER = "optim/unetpp_optim.h"                                   # relative to include/
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join("..", "..", "include", "optim", "unetpp_optim.h")]
# -ffp-contract=off: the header pins the arithmetic operation by operation, so no product may fuse into a following sum
CXXFLAGS = _lib.CXXFLAGS + ["-ffp-contract=off"]

KINDS = {"adam": 0, "adamw": 1, "sgd": 2}                         # UNETPP_OPTIM_*
MAX_GROUPS = 8


class Groups(ctypes.Structure):
    """unetpp_optim_groups: the param groups' end offsets and hyper-parameters, passed by value at every launch."""
    _fields_ = [("n_groups", ctypes.c_int32), ("kind", ctypes.c_int32), ("end", ctypes.c_int64 * MAX_GROUPS)] + [
        (n, ctypes.c_double * MAX_GROUPS) for n in ("lr", "beta1", "beta2", "eps", "weight_decay", "momentum")]


class StepArgs(ctypes.Structure):
    """unetpp_optim_step_args."""
    _fields_ = [("use_clip", ctypes.c_int32), ("max_norm", ctypes.c_float),
                ("growth_factor", ctypes.c_float), ("backoff_factor", ctypes.c_float), ("growth_interval", ctypes.c_int32),
                ("zero_grads", ctypes.c_int32), ("parity", ctypes.c_int32), ("scaler_parity", ctypes.c_int32)]


vp, ci, ip = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)

ABI_OPTIM = {
    "unetpp_optim_layout": (ci, [ip, ip, ip, ip]),
    "unetpp_optim_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "unetpp_optim_version": (ctypes.c_char_p, []),
    "unetpp_optim_grad_norm_f32": (ci, [vp, ctypes.c_int64, vp, vp]),
    "unetpp_optim_step_f32": (ci, [vp, vp, vp, vp, ctypes.c_int64, ctypes.POINTER(Groups), ctypes.POINTER(StepArgs), vp, vp, vp, vp]),
}

_TAG = b"(gfx950) osrc:"


def source_hash() -> str:
    """Digest of the library's sources, headers and compiler flags; unetpp_optim_version() ends in 'osrc:<hash>'."""
    h = hashlib.sha256()
    h.update(" ".join(CXXFLAGS).encode() + b"\0")
    for rel in sorted(SOURCES + HEADERS):
        with open(os.path.join(CSRC, rel), "rb") as f:
            h.update(rel.encode() + b"\0" + f.read() + b"\0")
    return h.hexdigest()[:16]


def built_hash(path: str = LIB_PATH):
    """The 'osrc:' tag of a built library, read from the file (no dlopen), or None."""
    try:
        with open(path, "rb") as f:
            blob = f.read()
    except OSError:
        return None
    i = blob.find(_TAG)
    return None if i < 0 else blob[i + len(_TAG):i + len(_TAG) + 16].decode("ascii", "replace")


def _stale() -> bool:
    return built_hash() != source_hash()


def build(force: bool = False, verbose: bool = False) -> str:
    """hipcc --offload-arch=gfx950 -> unet-_amd/libunetpp_optim_hip.so (cross-compiles without a GPU)."""
    if not force and not _stale():
        return LIB_PATH
    hipcc = _lib._hipcc()
    if not hipcc:
        raise RuntimeError("hipcc not found: cannot build libunetpp_optim_hip.so")
    tmp = f"{LIB_PATH}.{os.getpid()}.tmp"      # several ranks may build at once: write aside, then rename atomically
    cmd = [hipcc] + CXXFLAGS + ["-shared", "-fPIC", f'-DUNETPP_OPTIM_SRC_HASH="{source_hash()}"', "-o", tmp] + [
        os.path.join(CSRC, s) for s in SOURCES]
    if verbose:
        print(" ".join(cmd).replace(tmp, LIB_PATH), flush=True)
    try:
        subprocess.run(cmd, check=True, cwd=CSRC)
        os.replace(tmp, LIB_PATH)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return LIB_PATH


_loaded = None


def load(build_if_missing: bool = True) -> ctypes.CDLL:
    global _loaded
    if _loaded is not None:
        return _loaded
    _lib.share_torch_hip_runtime()
    if _stale():
        what = "is missing" if not os.path.exists(LIB_PATH) else f"was built from other sources (osrc:{built_hash()}, tree {source_hash()})"
        if not build_if_missing or not _lib._hipcc():
            raise RuntimeError(f"{LIB_PATH} {what}: build it with __graft_entry__.build(); there is no CPU fallback")
        build()
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in ABI_OPTIM.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    ver = lib.unetpp_optim_version().decode()
    if not ver.endswith("osrc:" + source_hash()):
        raise RuntimeError(f"{LIB_PATH} reports {ver!r}, tree is osrc:{source_hash()}")
    _loaded = lib
    return lib


def layout() -> dict:
    """{granule, max_partials, state_slot_words, max_groups} of unetpp_optim_layout."""
    out = [ctypes.c_int() for _ in range(4)]
    rc = load().unetpp_optim_layout(*[ctypes.byref(o) for o in out])
    if rc:
        raise RuntimeError(f"unetpp_optim_layout: {rc}")
    return dict(zip(("granule", "max_partials", "state_slot_words", "max_groups"), (o.value for o in out)))
