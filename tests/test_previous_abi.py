"""gv_pool_keep_models / gv_pool_forget_models / gv_pool_emit_previous and their readers on the CPU tier: the header declares the five
entry points with the signatures garden_amd/lib.py binds, the library exports them, GvPreviousLayout has the same size and offsets in
C99 and in ctypes, the flag values agree, the ABI version is still 4 (the change is additive), the rule's text stands word for word in
include/garden_vis.h, gv_device_math.hpp, tests/previous_twin.h and DESIGN.md; known answers of the C twin that can be worked out by
hand; and a census of the two-frame GPU cases (tests/previous_support.py) on the oracle: each class of draw — kept and unmoved, kept
and moved, fresh — holds what previous_support.class_floor asks of the case."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import previous_support as ps
import second_phase_support as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, U32 = C.c_void_p, C.c_uint32
OFFSETS = [("stride", 0), ("prev_mvp", 4), ("has_history", 8)]
IDENTITY = np.eye(4, dtype=np.float32).reshape(16)
MODEL_IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)


def signatures():
    from garden_amd import lib
    return {
        "gv_pool_keep_models": ("GvCtx* ctx, uint32_t pool_id, uint32_t view_index, uint32_t flags", [P, U32, U32, U32]),
        "gv_pool_forget_models": ("GvCtx* ctx, uint32_t pool_id, uint32_t first, uint32_t count", [P, U32, U32, U32]),
        "gv_pool_emit_previous": ("GvCtx* ctx, uint32_t pool_id, uint32_t view_index, const GvPreviousLayout* layout, const float* prev_view_proj, "
                                  "uint32_t flags, void* dst_device, size_t capacity_bytes",
                                  [P, U32, U32, C.POINTER(lib.GvPreviousLayout), C.POINTER(C.c_float), U32, P, C.c_size_t]),
        "gv_pool_previous_device": ("GvCtx* ctx, uint32_t pool_id, const void** items, const void** counts", [P, U32, C.POINTER(P), C.POINTER(P)]),
        "gv_pool_previous_fetch": ("GvCtx* ctx, uint32_t pool_id, void* dst_host, size_t bytes, uint32_t* counts4",
                                   [P, U32, P, C.c_size_t, C.POINTER(U32)]),
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
    assert re.search(r"#define GV_KEEP_ADD 1u?\b", text)
    assert re.search(r"#define GV_PREVIOUS_CUT 1u?\b", text)
    assert re.search(r"#define GV_ABI_VERSION 4u?\b", text)


def test_library_exports_them_and_lib_py_binds_the_same_signatures():
    from garden_amd import lib
    for name in signatures():
        assert name in lib.EXPORTS, name
    assert lib.GV_KEEP_ADD == 1 and lib.GV_PREVIOUS_CUT == 1
    assert C.sizeof(lib.GvPreviousLayout) == 12
    assert [(n, getattr(lib.GvPreviousLayout, n).offset) for n, _ in lib.GvPreviousLayout._fields_] == OFFSETS
    for method in ("keep_models", "forget_models", "emit_previous", "previous_device", "previous"):
        assert callable(getattr(lib.GpuVisibility, method)), method
    if os.path.exists(lib.LIB_PATH):
        handle = lib.load()
        assert handle.gv_abi_version() == 4
        for name, (_, argtypes) in signatures().items():
            fn = getattr(handle, name)
            assert list(fn.argtypes) == argtypes, name
            assert fn.restype in (C.c_int, C.c_int32), name


def test_header_compiles_as_c99_and_the_struct_has_these_offsets(tmp_path):
    src = tmp_path / "previous_abi.c"
    checks = "".join("typedef char %s_at_%d[offsetof(GvPreviousLayout, %s) == %d ? 1 : -1];\n" % (n, at, n, at) for n, at in OFFSETS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "garden_vis.h"\n'
                   "typedef char previous_layout_is_12_bytes[sizeof(GvPreviousLayout) == 12 ? 1 : -1];\n" + checks +
                   "typedef char abi_is_4[GV_ABI_VERSION == 4u ? 1 : -1];\n"
                   "typedef char flags_are_1[GV_KEEP_ADD == 1u && GV_PREVIOUS_CUT == 1u ? 1 : -1];\n"
                   "int main(void) {\n"
                   "    int (*keep)(GvCtx*, uint32_t, uint32_t, uint32_t) = gv_pool_keep_models;\n"
                   "    int (*forget)(GvCtx*, uint32_t, uint32_t, uint32_t) = gv_pool_forget_models;\n"
                   "    int (*emit)(GvCtx*, uint32_t, uint32_t, const GvPreviousLayout*, const float*, uint32_t, void*, size_t) = gv_pool_emit_previous;\n"
                   "    int (*dev)(GvCtx*, uint32_t, const void**, const void**) = gv_pool_previous_device;\n"
                   "    int (*fetch)(GvCtx*, uint32_t, void*, size_t, uint32_t*) = gv_pool_previous_fetch;\n"
                   "    GvPreviousLayout l = {64u, 0u, GV_NONE};\n"
                   '    printf("%u %d\\n", l.stride + l.prev_mvp, keep && forget && emit && dev && fetch);\n'
                   "    return 0;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "previous_abi.o")], check=True)


def rule_of(path):
    """the lines of the rule from 'THE PREVIOUS RULE' to the end of step 4, comment prefixes, list marks and indentation removed; the
    sentence in brackets that names the OTHER places the text stands in differs by construction and is cut"""
    lines, inside = [], False
    for line in open(os.path.join(ROOT, path)):
        if "THE PREVIOUS RULE" in line:
            inside = True
        if inside:
            lines.append(re.sub(r"^\s*(//|/?\*|>)?\s*", "", line.rstrip()))
            if "0 when fresh." in line:
                break
    text = " ".join(" ".join(lines).split())
    assert text.endswith("0 when fresh."), path
    return re.sub(r"\(the same text stands in [^)]*\)", "()", text).replace("**", "")


def test_the_rule_stands_word_for_word_in_every_place():
    texts = {path: rule_of(path) for path in ("include/garden_vis.h", "garden_amd/csrc/gv_device_math.hpp", "tests/previous_twin.h", "DESIGN.md")}
    first = texts["include/garden_vis.h"]
    assert "one fp32 add per component" in first and "Cut: GV_PREVIOUS_CUT, or e == 0" in first and "stamp[s_k] == e" in first
    for path, text in texts.items():
        assert text == first, path


def test_edge_sizes_follow_the_kernel_header():
    assert ps.header_constants() == ps.HEADER_NAMES
    for span in (64, ps.BLOCK):
        assert {span - 1, span, span + 1} <= set(ps.EDGE_DRAWS)
    assert {0, 1, ps.TILES * ps.BLOCK + 1} <= set(ps.EDGE_DRAWS) and max(ps.EDGE_DRAWS) < ps.EDGE_SLOTS


# ---- known answers of the twin -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return ps.build_twin(str(tmp_path_factory.mktemp("previous_twin")))


def view_of(view_proj=IDENTITY, camera=(0, 0, 0)):
    return dict(view_proj=np.asarray(view_proj, np.float32), camera_position=np.asarray(list(camera) + [0], np.float32))


def records(slots, models):
    models = np.asarray(models, np.float32).reshape(-1, 12)
    return dict(draw_count=len(models), visible_idx=np.asarray(slots, np.uint32), baked_model=models)


def completed(model):
    """the 4x4 (column-major) of a 12-float model"""
    out = np.zeros(16, np.float32)
    for j in range(4):
        out[4 * j:4 * j + 3] = model[3 * j:3 * j + 3]
    out[15] = 1
    return out


def test_identity_everywhere_gives_the_completed_model_and_an_empty_history_is_a_cut(twin):
    h = ps.History(twin)
    m = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], np.float32)
    mvp, has, kept = h.expect(view_of(camera=(5, 6, 7)), records([3], [m]))
    assert (has.tolist(), kept, h.epoch) == ([0], 0, 0)
    assert mvp[0].tolist() == completed(m).tolist()  # e == 0: d is 0 whatever the camera is
    h.keep(view_of(), records([3], [m]), occupancy=8)
    assert (h.epoch, h.slots) == (1, 8)
    moved = m.copy()
    moved[9:] += 100
    mvp, has, kept = h.expect(view_of(), records([3, 4], [moved, moved]))
    assert (has.tolist(), kept) == ([1, 0], 1)
    assert mvp[0].tolist() == completed(m).tolist()      # kept: the row, not this frame's model
    assert mvp[1].tolist() == completed(moved).tolist()  # fresh, the camera did not move


def test_fresh_draw_is_static_in_the_world_and_d_rounds_once(twin):
    h = ps.History(twin)
    h.keep(view_of(camera=(0, 0, 0)), records([], np.zeros((0, 12))), occupancy=4)
    m = MODEL_IDENTITY.copy()
    m[9:] = (2.0 ** 24, -3.0, 0.5)
    mvp, has, _ = h.expect(view_of(camera=(1, 1, 1)), records([0], [m]))
    # d = (1, 1, 1): 2^24 + 1 is a tie and rounds to even, 2^24; -3 + 1 and 0.5 + 1 are exact
    assert has.tolist() == [0] and mvp[0, 12:15].tolist() == [2.0 ** 24, -2.0, 1.5]
    m[9] = 2.0 ** 24 + 2
    assert h.expect(view_of(camera=(1, 1, 1)), records([0], [m]))[0][0, 12] == 2.0 ** 24 + 4  # 2^24 + 3: a tie again, to even
    # the kept camera is subtracted on the host in fp32: camera 0.1f - kept 0.3f
    h.keep(view_of(camera=(np.float32(0.3), 0, 0)), records([], np.zeros((0, 12))), occupancy=4)
    mvp, _, _ = h.expect(view_of(camera=(np.float32(0.1), 0, 0)), records([0], [MODEL_IDENTITY]))
    assert mvp[0, 12] == np.float32(0.0) + (np.float32(0.1) - np.float32(0.3))


def test_negative_zero_in_the_translation(twin):
    h = ps.History(twin)
    m = MODEL_IDENTITY.copy()
    m[9:] = (-0.0, -0.0, -0.0)
    # a cut: fresh with d = +0; -0 + +0 = +0, and the product's chains start from +0 either way: the bits emit_instances' mvp has
    mvp, _, _ = h.expect(view_of(), records([0], [m]))
    plain = np.empty(16, np.float32)
    twin.twin_mvp(IDENTITY.ctypes.data, m.ctypes.data, plain.ctypes.data)
    assert mvp[0].view(np.uint32).tolist() == plain.view(np.uint32).tolist()
    assert mvp[0, 12:15].view(np.uint32).tolist() == [0, 0, 0]
    # kept: the row is verbatim, -0 included (and gives the same product)
    h.keep(view_of(), records([0], [m]), occupancy=1)
    assert h.rows[0, 9:12].tolist() == [0x80000000] * 3 and h.rows[0, 12:].tolist() == [1, 0, 0, 0]
    mvp, has, _ = h.expect(view_of(), records([0], [MODEL_IDENTITY]))
    assert has.tolist() == [1] and mvp[0].view(np.uint32).tolist() == plain.view(np.uint32).tolist()


def test_infinite_view_proj_keeps_the_four_term_nesting(twin):
    h = ps.History(twin)
    vp = IDENTITY.copy()
    vp[12] = np.inf  # row 0 of the translation column
    m = MODEL_IDENTITY.copy()
    mvp, _, _ = h.expect(view_of(vp), records([0], [m]))
    # columns 0-2 multiply the infinity by b3 = 0: NaN in row 0; column 3 by 1: +inf
    assert np.isnan(mvp[0, [0, 4, 8]]).all() and mvp[0, 12] == np.inf
    assert mvp[0, [5, 10, 15]].tolist() == [1, 1, 1]
    # prev_view_proj, when given, replaces the kept matrix; under a cut the view's own is used
    h.keep(view_of(vp), records([0], [m]), occupancy=1)
    finite, _, _ = h.expect(view_of(vp), records([0], [m]), prev_view_proj=IDENTITY)
    assert finite[0].tolist() == completed(m).tolist()
    again, has, _ = h.expect(view_of(IDENTITY), records([0], [m]), prev_view_proj=vp, cut=True)
    assert has.tolist() == [0] and again[0].tolist() == completed(m).tolist()


def test_stamps_add_forget_and_wrap(twin):
    h = ps.History(twin)
    m = MODEL_IDENTITY
    h.keep(view_of(), records([0, 1], [m, m]), occupancy=4)
    h.keep(view_of(), records([1], [m]), occupancy=4)              # epoch 2: slot 0 is stale
    assert h.expect(view_of(), records([0, 1, 3], [m, m, m]))[1].tolist() == [0, 1, 0]
    h.keep(view_of(), records([2], [m]), occupancy=6, add=True)     # joins epoch 2; the coverage grows
    assert (h.epoch, h.slots) == (2, 6)
    assert h.expect(view_of(), records([0, 1, 2, 5, 6], [m] * 5))[1].tolist() == [0, 1, 1, 0, 0]
    h.forget(1, 100)
    assert h.expect(view_of(), records([0, 1, 2], [m] * 3))[1].tolist() == [0, 0, 0]
    h.keep(view_of(), records([0, 1], [m, m]), occupancy=6)
    h.h.epoch = 0xFFFFFFFF
    h.rows[0, 12] = 0xFFFFFFFF
    h.rows[1, 12] = 1                                               # would alias the epoch after the wrap
    h.keep(view_of(), records([2], [m]), occupancy=6)
    assert h.epoch == 1 and h.expect(view_of(), records([0, 1, 2], [m] * 3))[1].tolist() == [0, 0, 1]
    h.forget()
    assert (h.epoch, h.slots) == (0, 0)


# ---- the census of the GPU cases on the oracle -----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sp.CASES, ids=lambda c: c.name)
def test_every_two_frame_case_holds_every_class_of_draw(case):
    census, floor = ps.census(case.name), ps.class_floor(case)
    assert census.unmoved + census.moved + census.fresh == census.draws
    for name in ("unmoved", "moved", "fresh"):
        assert getattr(census, name) >= floor, (case.name, name, census, floor)


def test_the_floor_is_64_draws_wherever_the_case_can_hold_them():
    assert ps.CLASS_MIN == 64
    assert sum(ps.class_floor(c) == 64 for c in sp.CASES) >= 5 and all(ps.class_floor(c) == 64 for c in sp.CASES if c.n >= 5120)
    assert all(ps.class_floor(c) >= 1 for c in sp.CASES if c.n >= 256 and not c.empty)
