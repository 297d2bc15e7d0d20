"""gv_pool_draw_occluders and its companions on the CPU tier: the header declares the six entry points and GV_DIRTY_OCCLUDER with the
signatures garden_amd/lib.py binds, the library exports them, GvOccluderCounts is six words in C99 and in ctypes, the ABI version is
still 4 (the change is additive), the rule's text stands word for word in DESIGN.md, gv_device_math.hpp and tests/occluder_twin.h,
and the kernel header holds the tile and workgroup sizes the GPU cases are built from."""
import ctypes as C
import os
import re
import subprocess

import occluders_support as osup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, U32 = C.c_void_p, C.c_uint32


def signatures():
    from garden_amd import lib
    return {
        "gv_pool_bind_occluders": ("GvCtx* ctx, uint32_t pool_id, const void* box_min, const void* box_max, uint32_t stride, uint32_t occupancy",
                                   [P, U32, P, P, U32, U32]),
        "gv_occluder_begin": ("GvCtx* ctx, uint32_t width, uint32_t height", [P, U32, U32]),
        "gv_pool_draw_occluders": ("GvCtx* ctx, uint32_t pool_id, uint32_t view_index, uint32_t min_pixels", [P, U32, U32, U32]),
        "gv_occluder_depth_device": ("GvCtx* ctx, const void** depth, uint32_t* width, uint32_t* height, const void** counts",
                                     [P, C.POINTER(P), C.POINTER(U32), C.POINTER(U32), C.POINTER(P)]),
        "gv_occluder_depth_fetch": ("GvCtx* ctx, float* depth, size_t bytes, GvOccluderCounts* counts",
                                    [P, P, C.c_size_t, C.POINTER(lib.GvOccluderCounts)]),
        "gv_hiz_build_from_occluders": ("GvCtx* ctx", [P]),
    }


def header(comments=False):
    text = open(os.path.join(ROOT, "include", "garden_vis.h")).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_entry_points_with_these_signatures():
    text = header()
    for name, (params, _) in signatures().items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        assert " ".join(m.group(1).split()) == params, name
    assert re.search(r"\bGV_DIRTY_OCCLUDER\s*=\s*6\b", text)
    assert re.search(r"#define GV_ABI_VERSION 4u?\b", text)


def test_header_comment_states_the_binders_contract():
    text = " ".join(header(comments=True).replace("\n *", "\n").split())
    assert "THE BINDER'S CONTRACT: the library does not check that an occluder box lies inside the slot's AABB" in text


def test_library_exports_them_and_lib_py_binds_the_same_signatures():
    from garden_amd import lib
    for name in signatures():
        assert name in lib.EXPORTS, name
    assert lib.GV_DIRTY_OCCLUDER == 6
    assert C.sizeof(lib.GvOccluderCounts) == 24
    assert tuple(n for n, _ in lib.GvOccluderCounts._fields_) == osup.COUNT_NAMES == lib.OCCLUDER_COUNT_NAMES
    for method in ("bind_occluders", "occluder_begin", "draw_occluders", "occluder_depth", "occluder_depth_device", "hiz_build_from_occluders"):
        assert callable(getattr(lib.GpuVisibility, method)), method
    if os.path.exists(lib.LIB_PATH):
        handle = lib.load()
        assert handle.gv_abi_version() == 4
        for name, (_, argtypes) in signatures().items():
            fn = getattr(handle, name)
            assert list(fn.argtypes) == argtypes, name
            assert fn.restype in (C.c_int, C.c_int32), name


def test_header_compiles_as_c99_and_the_counts_are_six_words(tmp_path):
    src = tmp_path / "occluders_abi.c"
    checks = "".join("typedef char %s_at_%d[offsetof(GvOccluderCounts, %s) == %d ? 1 : -1];\n" % (n, 4 * i, n, 4 * i)
                     for i, n in enumerate(osup.COUNT_NAMES))
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "garden_vis.h"\n'
                   "typedef char counts_are_24_bytes[sizeof(GvOccluderCounts) == 24 ? 1 : -1];\n" + checks +
                   'int main(void) { printf("%d\\n", (int)GV_DIRTY_OCCLUDER); return 0; }\n')
    exe = tmp_path / "occluders_abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip() == "6"


def rule_text(path, prefix):
    """the lines of the rule between 'THE RULE' and item 9's last line, comment prefixes and indentation removed"""
    lines = open(os.path.join(ROOT, path)).read().split("\n")
    start = next(i for i, l in enumerate(lines) if "THE RULE" in l)
    end = next(i for i in range(start, len(lines)) if "does not depend on any order of evaluation" in lines[i])
    body = [re.sub(r"^\s*" + re.escape(prefix) + r" ?", "", l) for l in lines[start + 1:end + 1]]
    return " ".join(" ".join(body).split())


def test_the_rule_stands_word_for_word_in_all_three_places():
    twin = rule_text("tests/occluder_twin.h", "*")
    assert len(twin) > 2000 and "1. Has a box" in twin[:300] and "9. depth[py W + px]" in twin
    assert rule_text("garden_amd/csrc/gv_device_math.hpp", "//") == twin
    assert rule_text("DESIGN.md", "") == twin


def test_kernel_header_holds_the_sizes_the_cases_are_built_from():
    assert osup.T == 32 and osup.BLOCK == 256
    assert osup.IMAGE_SIZES[-1] == (2 * osup.T + 1, 2 * osup.T + 1)
    for n in (osup.BLOCK - 1, osup.BLOCK, osup.BLOCK + 1, 4 * osup.BLOCK + 1):
        assert n in osup.RECORD_COUNTS
