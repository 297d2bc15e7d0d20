"""The instance payload (gv_pool_bind_payload / gv_pool_set_payload_layout) on the CPU tier: the header declares both entry points
and the library exports them, the new enum value and macros are there, GvPayloadField has the C layout in ctypes, and the ABI
version is still 4 (the change is additive)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gv_pool_bind_payload", "gv_pool_set_payload_layout")


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "garden_vis.h")).read(), flags=re.S)


def test_header_declares_and_library_exports_the_entry_points():
    from garden_amd import lib
    text = header()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in lib.EXPORTS, name
    if os.path.exists(lib.LIB_PATH):
        handle = lib.load()
        for name in SYMBOLS:
            assert hasattr(handle, name), name
        assert handle.gv_abi_version() == 4
    assert re.search(r"#define GV_ABI_VERSION 4u?\b", text)


def test_enum_value_and_macros():
    from garden_amd import lib
    text = header()
    assert re.search(r"\bGV_DIRTY_PAYLOAD\s*=\s*3\b", text)
    assert re.search(r"#define GV_MAX_PAYLOAD_FIELDS 4u?\b", text)
    assert re.search(r"#define GV_MAX_PAYLOAD_BYTES 64u?\b", text)
    assert (lib.GV_DIRTY_PAYLOAD, lib.GV_MAX_PAYLOAD_FIELDS, lib.GV_MAX_PAYLOAD_BYTES) == (3, 4, 64)


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-pedantic"], ["g++", "-std=c++11", "-pedantic", "-x", "c++"]], ids=["c99", "cxx11"])
def test_payload_field_struct_and_constants_match_the_header(tmp_path, compiler):
    from garden_amd import lib
    cls = lib.GvPayloadField
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "garden_vis.h"', "int main(void) {",
             '    printf("%zu", sizeof(GvPayloadField));']
    for field, _ in cls._fields_:
        lines.append(f'    printf(" %zu", offsetof(GvPayloadField, {field}));')
    lines += ['    printf(" %u %u %u", (unsigned)GV_DIRTY_PAYLOAD, (unsigned)GV_MAX_PAYLOAD_FIELDS, (unsigned)GV_MAX_PAYLOAD_BYTES);',
              '    printf("\\n");', "    return 0;", "}"]
    src = tmp_path / "payload_abi.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "payload_abi"
    subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, *rest = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    offsets, constants = rest[:3], rest[3:]
    assert int(size) == ctypes.sizeof(cls) == 16
    assert [int(o) for o in offsets] == [getattr(cls, f).offset for f, _ in cls._fields_] == [0, 8, 12]
    assert [int(c) for c in constants] == [3, 4, 64]
