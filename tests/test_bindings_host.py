"""The C ABI bindings, checked once for every entry-point family (no GPU).  A family is a public header of include/, its
table in _lib.BINDINGS and its guard-band module; every test here runs once per header of _lib.BINDINGS:

  names           the header declares exactly the table's names
  build inputs    the header is hashed by _lib.source_hash() and reached by a source's #include chain
  definition      every symbol is defined in exactly one source, exported by the built library and typed by load()
  prototype       every argument and the return value of the C prototype against the table's ctypes entry, by count and by kind:
                  an argtypes entry is a hand transcription, and c_int where the header says int64_t truncates silently
  launching       an entry whose last parameter is the stream takes the engine first, and every entry a guard module does not
                  exclude is such an entry
  guard coverage  every symbol has a guard-band case or is excluded from them with a reason

What only one family has (enum values, layout numbers, source greps, required row names, C99 compile tests, null-engine return
codes) is in that family's own host test."""
import ctypes
import functools
import importlib
import os
import re

import pytest

from conftest import ROOT
from unet_amd import _lib

# the frozen number of symbols per header: an entry added to or taken from a header changes one number here
SIZES = {"unetpp.h": 76, "unetpp_roi.h": 8, "unetpp_loss.h": 2, "unetpp_contours.h": 5, "unetpp_simple_loops.h": 5, "unetpp_raw.h": 2,
         "unetpp_two_stage.h": 3, "unetpp_loss_grad.h": 3, "unetpp_train_batch.h": 3}

# header -> (its guard-band module, the names there that hold the covered symbols, the name of its exclusions); a list holds rows
# (Row.symbols), a dict or set holds symbols; None: the module excludes nothing (an empty dict)
GUARDED = {
    "unetpp.h": ("test_gpu_guarded", ("ROWS", "NETWORK_SYMBOLS"), "EXCLUDED"),
    "unetpp_roi.h": ("test_gpu_guarded_roi", ("ROWS_ROI",), "EXCLUDED_ROI"),
    "unetpp_loss.h": ("test_gpu_guarded_loss", ("ROWS_LOSS",), "EXCLUDED_LOSS"),
    "unetpp_contours.h": ("test_gpu_guarded_contours", ("ROWS_CONTOURS",), "EXCLUDED_CONTOURS"),
    "unetpp_simple_loops.h": ("test_gpu_guarded_simple_loops", ("ROWS_SIMPLE_LOOPS",), None),
    "unetpp_raw.h": ("test_gpu_guarded_raw", ("ROWS_RAW",), None),
    "unetpp_two_stage.h": ("test_gpu_guarded_two_stage", ("ROWS_TWO_STAGE",), None),
    "unetpp_loss_grad.h": ("test_gpu_guarded_loss_grad", ("COVERED",), "EXCLUDED_LOSS_GRAD"),
    "unetpp_train_batch.h": ("test_gpu_guarded_train_batch", ("COVERED",), "EXCLUDED_TRAIN_BATCH"),
}
# A row lists the symbols its call reaches (the harness compares them with the calls it saw), and these three wrappers ask for
# their workspace's size inside the call: the only names that are excluded and named by a row as well.
SIZE_QUERIES_ROWS_CALL = {"unetpp_roi_projection_workspace_bytes", "unetpp_roi_stats_workspace_bytes", "unetpp_contours_workspace_bytes"}

HEADERS = list(_lib.BINDINGS)
SCALARS = {"int": ("int", 4), "int64_t": ("int", 8), "long long": ("int", 8), "uint64_t": ("uint", 8), "uint8_t": ("uint", 1), "uint32_t": ("uint", 4),
           "size_t": ("uint", ctypes.sizeof(ctypes.c_size_t)), "float": ("float", 4), "double": ("float", 8)}


def without_comments(path):
    with open(path) as f:
        return re.sub(r"/\*.*?\*/|//[^\n]*", "", f.read(), flags=re.S)


@functools.lru_cache(maxsize=None)
def declared(header):
    """Every prototype of include/<header>, in order: (name, return type, [parameter, ...]), each as the header spells it."""
    protos = re.findall(r"^([A-Za-z_][\w \*]*?)\s*\b(unetpp_\w+)\s*\(([^()]*)\)\s*;", without_comments(os.path.join(ROOT, "include", header)), flags=re.M)
    return [(name, ret, [] if args.strip() == "void" else [" ".join(a.split()) for a in args.split(",")]) for ret, name, args in protos]


def c_kind(text, named):
    """A parameter (named) or a return type of a prototype: "pointer", None for void, or (class, bytes) of a scalar."""
    text = re.sub(r"\bconst\b", "", text)
    if "*" in text or "[" in text:
        return "pointer"
    base = " ".join(text.split()[:-1] if named else text.split())
    return None if base == "void" and not named else SCALARS[base]


def ctypes_kind(t):
    if t is None:
        return None
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "pointer"
    code = t._type_                                   # struct's format characters: f d, lower case signed, upper case unsigned
    return ("float" if code in "fd" else "int" if code.islower() else "uint", ctypes.sizeof(t))


@functools.lru_cache(maxsize=None)
def reached_by_the_sources():
    """The files the sources reach through #include "...", relative to csrc/ as _lib.HEADERS spells them; each must be hashed."""
    seen, todo = set(), list(_lib.SOURCES)
    while todo:
        rel = todo.pop()
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', without_comments(os.path.join(_lib.CSRC, rel)), flags=re.M):
            inc = os.path.relpath(os.path.normpath(os.path.join(_lib.CSRC, os.path.dirname(rel), inc)), _lib.CSRC)
            assert inc in _lib.HEADERS, f"{rel} includes {inc}, which source_hash() does not cover"
            if inc not in seen:
                seen.add(inc)
                todo.append(inc)
    return seen


def guard_tables(header):
    """(covered symbols, {excluded symbol: reason}, rows) of the header's guard-band module."""
    module, covered_in, excluded_in = GUARDED[header]
    mod = importlib.import_module(module)
    covered, rows = set(), []
    for attr in covered_in:
        value = getattr(mod, attr)
        if isinstance(value, list):
            rows += value
            covered |= set().union(*(r.symbols for r in value))
        else:
            covered |= set(value)
    return covered, (getattr(mod, excluded_in) if excluded_in else {}), rows


def check_guard_coverage(header):
    covered, excluded, rows = guard_tables(header)
    table = set(_lib.BINDINGS[header])
    bound = set().union(*_lib.BINDINGS.values())
    assert covered <= bound, sorted(covered - bound)
    assert set(excluded) <= table, sorted(set(excluded) - table)
    assert covered & set(excluded) == SIZE_QUERIES_ROWS_CALL & table, sorted(covered & set(excluded))
    assert (covered & table) | set(excluded) == table, f"neither guarded nor excluded: {sorted(table - covered - set(excluded))}"
    assert all(isinstance(why, str) and why for why in excluded.values())
    names = [r.name for r in rows]
    assert len(set(names)) == len(names), sorted(n for n in set(names) if names.count(n) > 1)


def test_the_registry_is_complete():
    assert list(SIZES) == HEADERS == list(GUARDED) and sum(SIZES.values()) == 107
    assert sorted(HEADERS) == sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))
    assert _lib.ABI_SYMBOLS == list(_lib.ABI) and _lib.BINDINGS["unetpp.h"] is _lib.ABI
    assert SIZE_QUERIES_ROWS_CALL <= set().union(*(guard_tables(h)[1] for h in HEADERS))
    assert reached_by_the_sources() == set(_lib.HEADERS)       # no header on disk that nothing includes, none included that is not hashed


def test_a_name_in_two_tables_is_refused_at_import():
    path = os.path.join(_lib._HERE, "_lib.py")
    with open(path) as f:
        text = f.read()
    assert text.count('"unetpp_loss_layout": (') == 1
    with pytest.raises(ImportError, match=r"bound in two tables of BINDINGS: \['unetpp_version'\]"):
        exec(compile(text.replace('"unetpp_loss_layout": (', '"unetpp_version": ('), path, "exec"), {"__name__": "_lib_copy", "__file__": path})


@pytest.mark.parametrize("header", HEADERS)
def test_header_and_table_hold_the_same_names(header):
    names = [name for name, _, _ in declared(header)]
    assert set(names) == set(_lib.BINDINGS[header]) and len(names) == len(_lib.BINDINGS[header]) == SIZES[header]


@pytest.mark.parametrize("header", HEADERS)
def test_header_is_a_build_input(header):
    rel = os.path.join("..", "..", "include", header)
    assert rel in _lib.HEADERS and os.path.isfile(os.path.join(_lib.CSRC, rel))
    assert rel in reached_by_the_sources()


@pytest.mark.parametrize("header", HEADERS)
def test_every_symbol_is_defined_once_exported_and_typed(header):
    sources = [without_comments(os.path.join(_lib.CSRC, s)) for s in _lib.SOURCES]
    lib = _lib.load()
    for name, (restype, argtypes) in _lib.BINDINGS[header].items():
        defined = [len(re.findall(r"^[A-Za-z_][\w \*]*\b%s\s*\([^()]*\)\s*\{" % name, text, flags=re.M)) for text in sources]
        assert sorted(defined) == [0] * (len(sources) - 1) + [1], (name, dict(zip(_lib.SOURCES, defined)))
        fn = getattr(lib, name)                                                     # AttributeError: not exported
        assert fn.restype is restype and fn.argtypes == argtypes, name


@pytest.mark.parametrize("header", HEADERS)
def test_prototypes_and_table_agree_in_every_argument(header):
    for name, ret, params in declared(header):
        restype, argtypes = _lib.BINDINGS[header][name]
        assert ctypes_kind(restype) == c_kind(ret, named=False), f"{name} returns {ret}, the table says {restype}"
        assert len(argtypes) == len(params), f"{name} takes {len(params)} arguments, the table has {len(argtypes)}"
        for i, (param, argtype) in enumerate(zip(params, argtypes)):
            assert ctypes_kind(argtype) == c_kind(param, named=True), f"{name}, argument {i}: the header says {param!r}, the table {argtype.__name__}"


@pytest.mark.parametrize("header", HEADERS)
def test_launching_entries_take_the_engine_first_and_the_stream_last(header):
    excluded = guard_tables(header)[1]
    for name, ret, params in declared(header):
        if params and params[-1] == "void* stream":
            assert params[0] == "unetpp_engine* e", name
        if name not in excluded:                       # what a guard-band case covers is a launch: a status code, the engine, ..., the stream
            assert ret == "int" and params[0] == "unetpp_engine* e" and params[-1] == "void* stream", name


@pytest.mark.parametrize("header", HEADERS)
def test_every_symbol_has_a_guard_case_or_a_stated_reason(header):
    check_guard_coverage(header)
