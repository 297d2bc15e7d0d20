"""gv_pool_draw_receivers and its companions on the CPU tier: the header declares the five entry points with the signatures
garden_amd/lib.py binds, the library exports them, GvReceiverCounts is six words in C99 and in ctypes, the ABI version is still 4 (the
change is additive), the rule's text stands word for word in DESIGN.md, gv_device_math.hpp and tests/receiver_twin.h — and item 16's
beside it is still the first rule in each — and the kernel header holds the sizes the GPU cases are built from."""
import ctypes as C
import os
import re
import subprocess

import receivers_support as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, U32 = C.c_void_p, C.c_uint32


def signatures():
    from garden_amd import lib
    return {
        "gv_receiver_begin": ("GvCtx* ctx, uint32_t width, uint32_t height", [P, U32, U32]),
        "gv_pool_draw_receivers": ("GvCtx* ctx, uint32_t pool_id, uint32_t view_index, const float light_view_proj[16]", [P, U32, U32, P]),
        "gv_receiver_mask_device": ("GvCtx* ctx, const void** mask, uint32_t* width, uint32_t* height, const void** counts",
                                    [P, C.POINTER(P), C.POINTER(U32), C.POINTER(U32), C.POINTER(P)]),
        "gv_receiver_mask_fetch": ("GvCtx* ctx, float* mask, size_t bytes, GvReceiverCounts* counts",
                                   [P, P, C.c_size_t, C.POINTER(lib.GvReceiverCounts)]),
        "gv_hiz_build_from_receivers": ("GvCtx* ctx", [P]),
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
    assert re.search(r"#define GV_ABI_VERSION 4u?\b", text)


def test_header_comment_states_the_frame_order_and_the_one_pyramid():
    text = " ".join(header(comments=True).replace("\n *", "\n").split())
    assert "gv_receiver_begin -> gv_pool_draw_receivers(pool, main view, L_k)" in text
    assert "gv_hiz_build_from_receivers -> gv_cull of cascade k with use_hiz = 1" in text
    assert "The context has ONE pyramid" in text and "leave the batched multi-view pass" in text


def test_library_exports_them_and_lib_py_binds_the_same_signatures():
    from garden_amd import lib
    for name in signatures():
        assert name in lib.EXPORTS, name
    assert C.sizeof(lib.GvReceiverCounts) == 24
    assert tuple(n for n, _ in lib.GvReceiverCounts._fields_) == rs.COUNT_NAMES == lib.RECEIVER_COUNT_NAMES
    for method in ("receiver_begin", "draw_receivers", "receiver_mask", "receiver_mask_device", "hiz_build_from_receivers"):
        assert callable(getattr(lib.GpuVisibility, method)), method
    if os.path.exists(lib.LIB_PATH):
        handle = lib.load()
        assert handle.gv_abi_version() == 4
        for name, (_, argtypes) in signatures().items():
            fn = getattr(handle, name)
            assert list(fn.argtypes) == argtypes, name
            assert fn.restype in (C.c_int, C.c_int32), name


def test_header_compiles_as_c99_and_the_counts_are_six_words(tmp_path):
    src = tmp_path / "receivers_abi.c"
    checks = "".join("typedef char %s_at_%d[offsetof(GvReceiverCounts, %s) == %d ? 1 : -1];\n" % (n, 4 * i, n, 4 * i)
                     for i, n in enumerate(rs.COUNT_NAMES))
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "garden_vis.h"\n'
                   "typedef char counts_are_24_bytes[sizeof(GvReceiverCounts) == 24 ? 1 : -1];\n" + checks +
                   "static int (*const draw)(GvCtx*, uint32_t, uint32_t, const float[16]) = gv_pool_draw_receivers;\n"
                   'int main(void) { printf("%d\\n", (int)sizeof(GvReceiverCounts) + (draw == 0)); return 0; }\n')
    exe = tmp_path / "receivers_abi.o"  # (compiled, not linked: the typedefs are the checks)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)


def rule_text(path, prefix, start_mark, end_mark):
    """the lines of a rule between the line that holds start_mark and the one that holds end_mark, comment prefixes and indentation removed"""
    lines = open(os.path.join(ROOT, path)).read().split("\n")
    start = next(i for i, l in enumerate(lines) if start_mark in l)
    end = next(i for i in range(start, len(lines)) if end_mark in lines[i])
    body = [re.sub(r"^\s*" + re.escape(prefix) + r" ?", "", l) for l in lines[start + 1:end + 1]]
    return " ".join(" ".join(body).split())


PLACES = (("tests/receiver_twin.h", "*"), ("garden_amd/csrc/gv_device_math.hpp", "//"), ("DESIGN.md", ""))


def test_the_rule_stands_word_for_word_in_all_three_places():
    texts = [rule_text(path, prefix, "THE RECEIVER RULE", "depends on no order of evaluation") for path, prefix in PLACES]
    assert len(texts[0]) > 2000 and "1. Corners p_c" in texts[0][:400] and "8. mask[py W + px]" in texts[0]
    assert texts[1] == texts[0] and texts[2] == texts[0]
    for step in range(1, 9):
        assert " %d. " % step in " " + texts[0], step


def test_item_16s_rule_is_still_the_first_rule_in_the_two_files_it_shares():
    twin = rule_text("tests/occluder_twin.h", "*", "THE RULE", "does not depend on any order of evaluation")
    for path, prefix in PLACES[1:]:
        assert rule_text(path, prefix, "THE RULE", "does not depend on any order of evaluation") == twin, path


def test_kernel_header_holds_the_sizes_the_cases_are_built_from():
    assert rs.T == 32 and rs.BLOCK == 256 and 1 <= rs.SMALL_PIXELS <= 32
    assert (2 * rs.T + 1, 2 * rs.T + 1) in rs.IMAGE_SIZES and (1, 1) in rs.IMAGE_SIZES
    for n in (rs.BLOCK - 1, rs.BLOCK, rs.BLOCK + 1, 4 * rs.BLOCK + 1):
        assert n in rs.RECORD_COUNTS
