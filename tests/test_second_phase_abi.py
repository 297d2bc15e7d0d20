"""gv_pool_cull_second_phase on the CPU tier: the header declares the entry point with the signature garden_amd/lib.py binds, the
library exports it, the ABI version is still 4 (the change is additive), the header says that the second view's is_visible is more
than its records — and a census of the GPU case table (tests/second_phase_support.py): its sizes are the kernel header's thresholds,
it holds every launch form of phase 1 and every configuration the issue names, and the oracle's own answer for every case meets the
condition that keeps the case from passing by accident."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import second_phase_support as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, U32 = C.c_void_p, C.c_uint32
NAME = "gv_pool_cull_second_phase"
PARAMS = "GvCtx* ctx, uint32_t pool_id, uint32_t first_view, uint32_t second_view, const GvView* view"


def header(comments=False):
    text = open(os.path.join(ROOT, "include", "garden_vis.h")).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_entry_point_with_this_signature():
    text = header()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, text)
    assert m, NAME
    assert " ".join(m.group(1).split()) == PARAMS
    assert re.search(r"#define GV_ABI_VERSION 4u?\b", text)


def test_header_comment_says_is_visible_is_the_union():
    text = header(comments=True)
    at = text.index("int " + NAME)
    comment = " ".join(text[text.rindex("/*", 0, at):at].split())
    assert "DELIBERATELY MORE THAN THE VIEW'S OWN RECORDS" in comment
    assert "S1" in comment and "emit_records must be 1" in comment


def test_library_exports_it_and_lib_py_binds_the_same_signature():
    from garden_amd import lib
    assert NAME in lib.EXPORTS
    assert callable(lib.GpuVisibility.cull_second_phase)
    if os.path.exists(lib.LIB_PATH):
        handle = lib.load()
        assert handle.gv_abi_version() == 4
        fn = getattr(handle, NAME)
        assert list(fn.argtypes) == [P, U32, U32, U32, C.POINTER(lib.GvView)]
        assert fn.restype in (C.c_int, C.c_int32)


def test_header_compiles_as_c99_with_the_new_declaration(tmp_path):
    src = tmp_path / "second_abi.c"
    src.write_text('#include <stdio.h>\n#include "garden_vis.h"\n'
                   "int main(void) {\n"
                   "    int (*second)(GvCtx*, uint32_t, uint32_t, uint32_t, const GvView*) = gv_pool_cull_second_phase;\n"
                   '    printf("%d\\n", second != 0);\n'
                   "    return 0;\n}\n")
    obj = tmp_path / "second_abi.o"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(obj)], check=True)


# ---- the census of the GPU case table ---------------------------------------------------------------------------------------------

def test_case_table_is_built_around_the_kernel_headers_constants():
    assert sp.header_constants() == sp.HEADER_NAMES
    assert sp.header_constant("gv_second_kernels.hpp", "kSecondBlock") == 256


def test_case_table_holds_every_launch_form_of_phase_one_and_every_configuration():
    flat = {c.n for c in sp.CASES if c.kind == "flat" and (c.w, c.h) == sp.SIZES[0] and not (c.keep_slot_order or c.rg16f)}
    assert {1, 64, 257, sp.EMIT_CHUNK + 1, 40000, 100003, 270000} <= flat
    assert 64 < 256 < 257                                  # below one cull tile, and one entry past it
    assert sp.EMIT_CHUNK + 1 <= sp.FUSED_EMIT_MAX < 40000  # one-launch cull + emit (no ballot words) | the ordinary launches
    assert 40000 <= sp.HOT_MIN < 100003                    # ... | the sphere-stream cull
    assert 100003 <= sp.AUTO_BOUNDS_MIN < 270000           # ... | block bounds
    odd = {c.n for c in sp.CASES if (c.w, c.h) == sp.SIZES[1]}
    assert {257, sp.EMIT_CHUNK + 1, 40000} <= odd
    kinds = {c.kind: c for c in sp.CASES}
    assert kinds["hierarchy"].n == 50000 and "shuffled" in kinds
    assert any(c.keep_slot_order for c in sp.CASES) and any(c.rg16f for c in sp.CASES)
    assert [c.name for c in sp.CASES if c.empty] == ["flat-1"]
    assert len({c.name for c in sp.CASES}) == len(sp.CASES)


@pytest.mark.parametrize("case", sp.CASES, ids=lambda c: c.name)
def test_every_case_meets_the_condition_on_the_oracle(case):
    """new, gone and both each hold a slot and 2 % of the frustum survivors; the expected second view is R minus S1 with the union
    bytes, and holds no slot of S1"""
    e = sp.expected(case.name)
    sp.check_condition(case, e)
    second = e.second
    assert second["draw_count"] == e.new == len(second["visible_idx"])
    assert not np.isin(second["visible_idx"], e.first["visible_idx"]).any()
    assert int(second["is_visible"].sum()) == e.new + e.gone + e.both
    assert (np.diff(second["visible_idx"].astype(np.int64)) > 0).all()
    if not case.empty:
        assert e.frustum > e.full["draw_count"] > e.new  # the pyramid occludes, and R is not all new
