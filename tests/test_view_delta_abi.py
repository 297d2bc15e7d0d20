"""gv_pool_view_delta and its companions on the CPU tier: the header declares the three entry points with the signatures
garden_amd/lib.py binds, the library exports them, GvViewDelta has the same size and offsets in C99 and in ctypes, the ABI version is
still 4 (the change is additive), the Python methods exist; and a census of the GPU cases (tests/view_delta_support.py) on the oracle:
the constants the edge sizes are built from are the kernel header's, and in every case appeared, vanished and stayed each hold a slot
and 2 % of the frustum survivors, the declared empty case excepted."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import second_phase_support as sp
import view_delta_support as vd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, U32 = C.c_void_p, C.c_uint32
OFFSETS = [("appeared", 0), ("vanished", 8), ("appeared_count", 16), ("vanished_count", 20), ("visible_count", 24), ("slots", 28)]


def signatures():
    from garden_amd import lib
    return {
        "gv_pool_view_delta": ("GvCtx* ctx, uint32_t pool_id, uint32_t channel, const uint32_t* view_indices, uint32_t view_count, uint32_t flags",
                               [P, U32, U32, C.POINTER(U32), U32, U32]),
        "gv_pool_view_delta_device": ("GvCtx* ctx, uint32_t pool_id, uint32_t channel, const void** slots, const void** counts",
                                      [P, U32, U32, C.POINTER(P), C.POINTER(P)]),
        "gv_pool_view_delta_fetch": ("GvCtx* ctx, uint32_t pool_id, uint32_t channel, int write_back, GvViewDelta* out",
                                     [P, U32, U32, C.c_int, C.POINTER(lib.GvViewDelta)]),
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
    assert re.search(r"#define GV_MAX_DELTA_CHANNELS 4u?\b", text)
    assert re.search(r"#define GV_DELTA_RESTART 1u?\b", text)
    assert re.search(r"#define GV_ABI_VERSION 4u?\b", text)


def test_header_comment_states_the_write_back_contract():
    text = header(comments=True)
    at = text.index("int gv_pool_view_delta_fetch")
    comment = " ".join(text[text.rindex("/*", 0, at):at].replace("\n *", "\n").split())
    assert "only if they held the BASELINE before" in comment and "GV_DELTA_RESTART call over zeroed bytes" in comment
    assert "nobody else writes those bytes in between" in comment and "touches NO other byte" in comment


def test_library_exports_them_and_lib_py_binds_the_same_signatures():
    from garden_amd import lib
    for name in signatures():
        assert name in lib.EXPORTS, name
    assert lib.GV_MAX_DELTA_CHANNELS == 4 and lib.GV_DELTA_RESTART == 1
    assert C.sizeof(lib.GvViewDelta) == 32
    assert [(n, getattr(lib.GvViewDelta, n).offset) for n, _ in lib.GvViewDelta._fields_] == OFFSETS
    for method in ("view_delta", "view_delta_issue", "view_delta_fetch", "view_delta_device", "view_delta_drop"):
        assert callable(getattr(lib.GpuVisibility, method)), method
    if os.path.exists(lib.LIB_PATH):
        handle = lib.load()
        assert handle.gv_abi_version() == 4
        for name, (_, argtypes) in signatures().items():
            fn = getattr(handle, name)
            assert list(fn.argtypes) == argtypes, name
            assert fn.restype in (C.c_int, C.c_int32), name


def test_header_compiles_as_c99_and_the_struct_has_these_offsets(tmp_path):
    src = tmp_path / "delta_abi.c"
    checks = "".join("typedef char %s_at_%d[offsetof(GvViewDelta, %s) == %d ? 1 : -1];\n" % (n, at, n, at) for n, at in OFFSETS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "garden_vis.h"\n'
                   "typedef char view_delta_is_32_bytes[sizeof(GvViewDelta) == 32 ? 1 : -1];\n" + checks +
                   "typedef char abi_is_4[GV_ABI_VERSION == 4u ? 1 : -1];\n"
                   "int main(void) {\n"
                   "    int (*issue)(GvCtx*, uint32_t, uint32_t, const uint32_t*, uint32_t, uint32_t) = gv_pool_view_delta;\n"
                   "    int (*dev)(GvCtx*, uint32_t, uint32_t, const void**, const void**) = gv_pool_view_delta_device;\n"
                   "    int (*fetch)(GvCtx*, uint32_t, uint32_t, int, GvViewDelta*) = gv_pool_view_delta_fetch;\n"
                   "    GvViewDelta d = {0, 0, 1u, 2u, 3u, 4u};\n"
                   '    printf("%u %u %u %d\\n", (unsigned)GV_MAX_DELTA_CHANNELS, (unsigned)GV_DELTA_RESTART, d.appeared_count + d.slots, issue && dev && fetch);\n'
                   "    return 0;\n}\n")
    obj = tmp_path / "delta_abi.o"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(obj)], check=True)


# ---- the census of the GPU cases on the oracle ------------------------------------------------------------------------------------

def test_edge_sizes_follow_the_kernel_header():
    assert vd.header_constants() == vd.HEADER_NAMES
    assert vd.WAVE == 64 * vd.WORD and vd.GROUP == vd.BLOCK * vd.WORD
    for span in (vd.WORD, vd.WAVE, vd.GROUP):
        assert {span - 1, span, span + 1} <= set(vd.EDGE_SIZES)
    assert 2 * vd.GROUP + 1 in vd.EDGE_SIZES and vd.BLOCK + 1 in vd.EDGE_SIZES


def check_shares(what, previous, current, frustum):
    appeared, vanished = vd.delta(previous, current)
    stayed = np.intersect1d(previous, current)
    for name, part in (("appeared", appeared), ("vanished", vanished), ("stayed", stayed)):
        assert len(part) >= 1 and len(part) >= vd.MIN_SHARE * frustum, (what, name, len(part), frustum)


@pytest.mark.parametrize("case", sp.CASES, ids=lambda c: c.name)
def test_every_case_of_the_table_changes_between_its_two_frames(case):
    e = sp.expected(case.name)
    first, full = vd.case_sets(case.name)
    if case.empty:
        assert len(first) == len(full) == 0
        return
    check_shares(case.name, first, full, e.frustum)
    assert (np.diff(first.astype(np.int64)) > 0).all() and (np.diff(full.astype(np.int64)) > 0).all()


@pytest.mark.parametrize("n", vd.EDGE_SIZES)
def test_every_edge_world_changes_between_its_two_cameras(n):
    """... and in the world of more than two workgroup spans both lists hold slots of several spans: a base crosses a workgroup. The
    enclosing view, the third frame of the GPU test, holds the last slot of every world but the ones whose last slot is a defect."""
    first, second = vd.edge_sets(n)
    check_shares(n, first, second, max(len(first), len(second)))
    if n > 2 * vd.GROUP:
        appeared, vanished = vd.delta(first, second)
        assert len(set((appeared // vd.GROUP).tolist())) >= 2 and len(set((vanished // vd.GROUP).tolist())) >= 2
    everything = vd.enclosed_set(n)
    assert len(everything) > 0.9 * n and len(np.setdiff1d(everything, second)) > len(second)
