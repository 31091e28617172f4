"""What the CPU tests of the C ABI share (test_abi_header.py and the test_abi_*.py of the extension headers): the C compiler, the
generated-C layout check of one extension struct, and the refusal of one entry point read three ways."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from vivim_amd import _lib

INCLUDE = os.path.join(ROOT, "include")
PTR = 4096          # a 16-byte aligned non-null "address": nothing is launched, so nothing reads it


def compiler():
    cc = shutil.which("cc")
    if cc:
        return [cc]
    makefile = open(os.path.join(ROOT, "vivim_amd", "csrc", "Makefile")).read()
    m = re.search(r"^HIPCC\s*[?:]?=\s*(\S+)", makefile, flags=re.M)
    hipcc = shutil.which(m[1] if m else "hipcc") or shutil.which("hipcc")
    return [hipcc, "-x", "c"] if hipcc else None


def layout_matches_c(header_file, c_name, cls, tmp_path):
    """The generated-C method of test_abi_header.py::test_layouts_match_the_c_compiler for the struct `c_name` of include/<header_file>:
    sizeof and every field's offsetof / sizeof as the compiler sees the header are those of `cls`, and no field leaves a hole."""
    cc = compiler()
    if cc is None:
        pytest.skip("no C compiler (neither cc nor the Makefile's hipcc)")
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header_file}"', "int main(void) {",
             f'    printf("- %zu\\n", sizeof({c_name}));']
    for field, _ in cls._fields_:
        lines.append(f'    printf("{field} %zu %zu\\n", offsetof({c_name}, {field}), sizeof((({c_name} *)0)->{field}));')
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(cc + ["-I", INCLUDE, "-o", str(exe), str(src)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert out[:-1] == [f"- {ctypes.sizeof(cls)}"] + [f"{n} {getattr(cls, n).offset} {getattr(cls, n).size}" for n, _ in cls._fields_]
    end = 0
    for n, _ in cls._fields_:                                # explicit padding, no holes
        assert getattr(cls, n).offset == end, n
        end += getattr(cls, n).size
    assert ctypes.sizeof(cls) == end


def refused(name, p, code=1):
    """The refusal of `name` for `p`: its return code directly, and its text both directly and through _lib.call."""
    L = _lib.lib()
    assert getattr(L, name)(ctypes.byref(p) if p is not None else None, None) == code
    direct = L.vivim_last_error().decode()
    if p is not None:
        with pytest.raises(RuntimeError) as info:
            _lib.call(name, p, 0)
        assert str(info.value) == direct
    assert direct
    return direct
