"""The optimiser library's bindings (include/optim/unetpp_optim.h, unet_amd/_lib_optim.py), without a GPU: the checks
tests/test_bindings_host.py runs per header of the engine's library, for the second library and its own loader."""
import ctypes
import os
import re

from conftest import ROOT
from test_bindings_host import c_kind, ctypes_kind, declared, without_comments
from unet_amd import _lib, _lib_optim, optim

HEADER = _lib_optim.HEADER


def test_header_and_table_hold_the_same_names():
    names = [name for name, _, _ in declared(HEADER)]
    assert names == list(_lib_optim.ABI_OPTIM) and len(names) == 5
    assert not set(names) & set().union(*_lib.BINDINGS.values())           # nothing bound in both libraries


def test_prototypes_and_table_agree_in_every_argument():
    for name, ret, params in declared(HEADER):
        restype, argtypes = _lib_optim.ABI_OPTIM[name]
        assert ctypes_kind(restype) == c_kind(ret, named=False), f"{name} returns {ret}, the table says {restype}"
        assert len(argtypes) == len(params), f"{name} takes {len(params)} arguments, the table has {len(argtypes)}"
        for i, (param, argtype) in enumerate(zip(params, argtypes)):
            assert ctypes_kind(argtype) == c_kind(param, named=True), f"{name}, argument {i}: the header says {param!r}, the table {argtype.__name__}"


def test_launching_entries_take_no_engine_and_the_stream_last():
    for name, ret, params in declared(HEADER):
        assert not any("unetpp_engine" in p for p in params), name
        if name.endswith("_f32"):
            assert ret == "int" and params[-1] == "void* stream", name


def struct_fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            ctype, rest = decl.split(" ", 1)
            fields += [(ctype, f.strip()) for f in rest.split(",")]
    return fields


def test_the_structs_match_the_header_field_by_field():
    text = without_comments(os.path.join(ROOT, "include", HEADER))
    kinds = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "float": ctypes.c_float}
    for cname, cls in (("unetpp_optim_groups", _lib_optim.Groups), ("unetpp_optim_step_args", _lib_optim.StepArgs)):
        want = []
        for ctype, field in struct_fields(text, cname):
            array = field.endswith("[UNETPP_OPTIM_MAX_GROUPS]")
            want.append((field.split("[")[0], kinds[ctype] * _lib_optim.MAX_GROUPS if array else kinds[ctype]))
        assert [(n, t) for n, t in cls._fields_] == want, cname
    assert re.search(r"UNETPP_OPTIM_MAX_GROUPS = (\d+)", text).group(1) == str(_lib_optim.MAX_GROUPS)
    enum = dict(re.findall(r"UNETPP_OPTIM_(ADAMW|ADAM|SGD) = (\d)", text))
    assert {k.lower(): int(v) for k, v in enum.items()} == _lib_optim.KINDS


def test_sources_and_headers_are_hashed_and_nothing_leaks_into_the_engines_library():
    assert os.path.isfile(os.path.join(_lib_optim.CSRC, _lib_optim.SOURCES[0]))
    seen, todo = set(), list(_lib_optim.SOURCES)
    while todo:
        rel = todo.pop()
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', without_comments(os.path.join(_lib_optim.CSRC, rel)), flags=re.M):
            inc = os.path.relpath(os.path.normpath(os.path.join(_lib_optim.CSRC, os.path.dirname(rel), inc)), _lib_optim.CSRC)
            assert inc in _lib_optim.HEADERS, f"{rel} includes {inc}, which source_hash() does not cover"
            if inc not in seen:
                seen.add(inc)
                todo.append(inc)
    assert seen == set(_lib_optim.HEADERS)
    assert "-ffp-contract=off" in _lib_optim.CXXFLAGS and _lib_optim.CXXFLAGS[:len(_lib.CXXFLAGS)] == _lib.CXXFLAGS
    assert not any("optim" in h for h in _lib.HEADERS)


def test_the_library_builds_for_gfx950_and_reports_its_source_hash():
    path = _lib_optim.build()
    assert path == _lib_optim.LIB_PATH and _lib_optim.built_hash() == _lib_optim.source_hash()
    lib = _lib_optim.load()
    ver = lib.unetpp_optim_version().decode()
    assert "(gfx950)" in ver and ver.endswith("osrc:" + _lib_optim.source_hash())
    for name, (restype, argtypes) in _lib_optim.ABI_OPTIM.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes == argtypes
    with open(path, "rb") as f:
        assert b"gfx950" in f.read()


def test_layout_and_workspace_are_what_optim_py_assumes():
    assert _lib_optim.layout() == {"granule": optim.GRANULE, "max_partials": optim.MAX_PARTIALS, "state_slot_words": optim.SLOT_WORDS,
                                   "max_groups": optim.MAX_GROUPS}
    lib = _lib_optim.load()
    for n in (1, 5, optim.GRANULE, optim.GRANULE + 1, 9_000_000, optim.GRANULE * optim.MAX_PARTIALS + 1, optim.MAX_N):
        assert lib.unetpp_optim_workspace_bytes(n) == optim.workspace_bytes(n), n
    assert lib.unetpp_optim_workspace_bytes(0) == 0 and lib.unetpp_optim_workspace_bytes(optim.MAX_N + 1) == 0


def test_bad_arguments_are_answered_before_any_launch():
    lib = _lib_optim.load()
    G, A = _lib_optim.Groups(), _lib_optim.StepArgs()
    G.n_groups, G.kind, G.end[0] = 1, 0, 64
    ok = (256, 512, 768, 1024, 64, ctypes.byref(G), ctypes.byref(A), 2048, 4096, None, None)
    assert lib.unetpp_optim_grad_norm_f32(None, 64, 2048, None) == -1
    assert lib.unetpp_optim_grad_norm_f32(256, 0, 2048, None) == -2
    assert lib.unetpp_optim_grad_norm_f32(258, 64, 2048, None) == -2            # not 4-byte aligned
    assert lib.unetpp_optim_grad_norm_f32(256, 64, 2052, None) == -2            # workspace not 8-byte aligned

    def step(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return lib.unetpp_optim_step_f32(*args)
    assert step(a0=None) == -1 and step(a2=None) == -1 and step(a3=None) == -1 and step(a8=None) == -1
    assert step(a4=65) == -2                                                   # the last group does not end at n
    assert step(a1=514) == -2 and step(a9=4098) == -2
    G.n_groups = 9
    assert step() == -2
    G.n_groups, G.kind = 1, 3
    assert step() == -2
    G.kind, A.parity = 0, 2
    assert step() == -2
    A.parity, A.growth_interval = 0, 0
    assert step(a9=8192) == -2                                                 # a scaler with growth_interval < 1
