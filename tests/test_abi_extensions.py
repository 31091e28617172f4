"""CPU: the registry of extension headers as a whole (vivim_amd/_lib.py: EXTENSIONS, load_extensions).  Version 8 is untouched; the rows
are exact, in order and disjoint; lib() binds all 60 names; the loader refuses, naming the header, what a row may not declare."""
import ctypes
import os

import pytest

import test_abi_header as th
from abi_cases import INCLUDE
from vivim_amd import _lib

ROWS = {    # file: (C struct -> Python class, entry points in header order, the word of the feature)
    "vivim_hip_ext.h": ({"vivim_structure_loss_params": "StructureLossParams"},
                        ("vivim_structure_loss_workspace_bytes", "vivim_structure_loss_fwd", "vivim_structure_loss_bwd"), "structure"),
    "vivim_hip_ext_head.h": ({"vivim_head_concat_params": "HeadConcatParams"},
                             ("vivim_head_concat_fwd", "vivim_head_concat_bwd"), "head_concat"),
    "vivim_hip_ext_binary_metrics.h": ({"vivim_binary_metrics_params": "BinaryMetricsParams"},
                                       ("vivim_binary_metrics_workspace_bytes", "vivim_binary_metrics"), "binary_metrics")}
TEXT = {file: open(os.path.join(INCLUDE, file)).read() for file in ["vivim_hip.h", *ROWS]}
X_H, Y_H, X = "vivim_hip_ext_x.h", "vivim_hip_ext_y.h", {"vivim_x_params": "XParams"}
GOOD = ("#ifndef VIVIM_HIP_EXT_X_H\n#define VIVIM_HIP_EXT_X_H\ntypedef struct { int32_t struct_bytes, n; void *out; } vivim_x_params;\n"
        "int vivim_x(const vivim_x_params *p, void *stream);\n#endif\n")
GOOD_Y = GOOD.replace("_X_", "_Y_").replace("vivim_x", "vivim_y")


def test_version_8_is_untouched():
    assert _lib.ABI_VERSION == 8 and len(_lib.ENTRY_POINTS) == 53 and len(_lib.STRUCT_NAMES) == 20 and len(_lib.STRUCTS) == 15
    assert list(_lib.STRUCT_NAMES.values()) == list(th.LAYOUTS) and [c.__name__ for c in _lib.STRUCTS] == th.STRUCTS
    assert set(_lib.ENTRY_POINTS) == set(th.ENTRIES) and _lib.EXPORTS == tuple(_lib.ENTRY_POINTS)
    assert not any(word in TEXT["vivim_hip.h"] for word in ("structure", "head_concat", "binary_metrics"))


def test_the_rows_are_exact_in_order_and_disjoint():
    assert list(_lib.EXTENSIONS) == list(ROWS) and sorted(os.listdir(INCLUDE)) == sorted(TEXT)       # one row per header file
    union = dict(_lib.ENTRY_POINTS)
    for file, (struct_names, names, word) in ROWS.items():
        got_names, entries = _lib.EXTENSIONS[file]
        assert got_names == struct_names and tuple(entries) == names and not set(entries) & set(union), file
        union.update(entries)
        for py in struct_names.values():
            cls = getattr(_lib, py)                                                                    # an attribute of _lib
            assert cls._fields_[0] == ("struct_bytes", ctypes.c_int32) and cls not in _lib.STRUCTS and py not in _lib.STRUCT_NAMES.values()
            assert all(e.struct is None and e.extra == (ctypes.POINTER(cls),) for e in entries.values())
        for other, text in TEXT.items():                         # the feature's names: in its own header and in none of the other three
            found = [n for n in (word, *struct_names, *names) if n in text]
            assert found == ([word, *struct_names, *names] if other == file else []), (file, other)
    assert _lib.ALL_ENTRY_POINTS == union and list(_lib.ALL_ENTRY_POINTS) == list(union) and len(union) == 53 + 3 + 2 + 2 == 60


def test_lib_binds_every_name_of_every_table_as_its_entry_dictates():
    L = _lib.lib()
    for name, e in _lib.ALL_ENTRY_POINTS.items():
        want = ([ctypes.POINTER(e.struct)] if e.struct else []) + list(e.extra) + ([ctypes.c_void_p] if e.stream else [])
        assert getattr(L, name).argtypes == want and getattr(L, name).restype is e.restype, name
    assert len(_lib.ALL_ENTRY_POINTS) == 60


def _load(tmp_path, headers):
    """load_extensions over `headers`, {file: (text or None for no file, struct names)}, written into tmp_path, beside the module's own names."""
    for file, (text, _) in headers.items():
        if text is not None:
            (tmp_path / file).write_text(text)
    rows = {file: (names, {}) for file, (_, names) in headers.items()}
    return rows, _lib.load_extensions(rows, str(tmp_path), _lib.ENTRY_POINTS, vars(_lib))


def test_the_loader_returns_what_it_parsed_and_fills_the_rows_in(tmp_path):
    rows, (classes, entries) = _load(tmp_path, {X_H: (GOOD, X), Y_H: (GOOD_Y, {"vivim_y_params": "YParams"})})
    assert list(classes) == ["XParams", "YParams"] and list(entries) == ["vivim_x", "vivim_y"]
    assert entries["vivim_x"] == _lib.Entry(None, (ctypes.POINTER(classes["XParams"]),), True, ctypes.c_int)
    assert rows[X_H][1] == {"vivim_x": entries["vivim_x"]} and rows[Y_H][1] == {"vivim_y": entries["vivim_y"]}
    assert not hasattr(_lib, "XParams") and "vivim_x" not in _lib.ALL_ENTRY_POINTS                     # the module's tables are not touched


@pytest.mark.parametrize("what, headers, error, message", [
    ("a struct that does not open with struct_bytes", {X_H: (GOOD.replace("struct_bytes", "batch"), X)}, ImportError,
     r"^vivim_hip_ext_x\.h: XParams does not open with struct_bytes"),
    ("a function of version 8", {X_H: (GOOD.replace("int vivim_x(", "int vivim_dir_gather("), X)}, ImportError,
     r"^vivim_hip_ext_x\.h: another header already declares vivim_dir_gather$"),
    ("a function of an earlier row", {X_H: (GOOD, X), Y_H: (GOOD_Y.replace("vivim_y(", "vivim_x("), {"vivim_y_params": "YParams"})}, ImportError,
     r"^vivim_hip_ext_y\.h: another header already declares vivim_x$"),
    ("a Python name of version 8", {X_H: (GOOD, {"vivim_x_params": "SsmFwdParams"})}, ImportError, r"^vivim_hip_ext_x\.h: .*\bSsmFwdParams\b"),
    ("a Python name that is another attribute of the module", {X_H: (GOOD, {"vivim_x_params": "lib"})}, ImportError, r"^vivim_hip_ext_x\.h: .*\blib\b"),
    ("a Python name of an earlier row", {X_H: (GOOD, X), Y_H: (GOOD_Y, {"vivim_y_params": "XParams"})}, ImportError, r"^vivim_hip_ext_y\.h: .*\bXParams\b"),
    ("a missing file", {X_H: (None, X)}, ImportError, r"vivim_hip_ext_x\.h cannot be read"),
    ("an unknown field type", {X_H: (GOOD.replace("void *out;", "unsigned flags;"), X)}, ValueError, r"^vivim_hip_ext_x\.h: unknown type"),
    ("a struct without a Python name", {X_H: (GOOD, {})}, ValueError, r"^vivim_hip_ext_x\.h: a struct without a Python name"),
    ("an unknown directive", {X_H: ("#pragma once\n" + GOOD, X)}, ValueError, r"^vivim_hip_ext_x\.h: a preprocessor line it does not know"),
])
def test_the_loader_refuses_naming_the_header(tmp_path, what, headers, error, message):
    with pytest.raises(error, match=message) as info:
        _load(tmp_path, headers)
    assert "vivim_hip.h" not in str(info.value) and (what != "a missing file" or str(tmp_path / X_H) in str(info.value))
    for text, names in headers.values() if error is ValueError else ():                                # the default name stays
        with pytest.raises(ValueError, match=r"^vivim_hip\.h: "):
            _lib.parse_header(text, names)
