"""gv_pool_emit_draw_commands and its companions on the CPU tier: the header declares the entry points with the signatures
garden_amd/lib.py binds, the library exports them, the new constants are there, the ABI version is still 4 (the change is additive),
and the numpy restatement of the rule the GPU tests compare against (tests/commands_support.py) gives three hand-written known
answers byte for byte."""
import ctypes as C
import os
import re
import struct

import numpy as np

import commands_support as csup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P, U32, SZ = C.c_void_p, C.c_uint32, C.c_size_t


def signatures():
    from garden_amd import lib
    # name -> (the parameter list of the header, whitespace squeezed; the argtypes lib.py must bind)
    return {
        "gv_pool_bind_geometry": (
            "GvCtx* ctx, uint32_t pool_id, const void* ids, uint32_t stride, uint32_t width, uint32_t occupancy, const GvGeometry* table, "
            "uint32_t table_count", [P, U32, P, U32, U32, U32, C.POINTER(lib.GvGeometry), U32]),
        "gv_pool_set_command_layout": ("GvCtx* ctx, uint32_t pool_id, const GvCommandLayout* layout", [P, U32, C.POINTER(lib.GvCommandLayout)]),
        "gv_pool_emit_draw_commands": (
            "GvCtx* ctx, uint32_t pool_id, uint32_t flags, uint32_t region_commands, void* dst_device, size_t capacity_bytes",
            [P, U32, U32, U32, P, SZ]),
        "gv_pool_draw_commands_device": ("GvCtx* ctx, uint32_t pool_id, const void** commands, const void** command_counts",
                                         [P, U32, C.POINTER(P), C.POINTER(P)]),
        "gv_pool_draw_commands_fetch": (
            "GvCtx* ctx, uint32_t pool_id, void* dst_host, size_t bytes, uint32_t* command_counts, uint32_t counts_capacity",
            [P, U32, P, SZ, C.POINTER(U32), U32]),
    }


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "garden_vis.h")).read(), flags=re.S)


def test_header_declares_the_entry_points_with_these_signatures():
    text = header()
    for name, (params, _) in signatures().items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        assert " ".join(m.group(1).split()) == params, name
    assert re.search(r"#define GV_MAX_GEOMETRIES 65536u?\b", text)
    assert re.search(r"#define GV_COMMANDS_MERGE_RUNS 1u?\b", text)
    assert re.search(r"\bGV_DIRTY_GEOMETRY = 4\b", text)
    assert re.search(r"#define GV_ABI_VERSION 4u?\b", text)


def test_library_exports_them_and_lib_py_binds_the_same_signatures():
    from garden_amd import lib
    for name in signatures():
        assert name in lib.EXPORTS, name
    assert lib.GV_MAX_GEOMETRIES == 65536 and lib.GV_DIRTY_GEOMETRY == 4 and lib.GV_COMMANDS_MERGE_RUNS == 1
    assert C.sizeof(lib.GvGeometry) == 12 and C.sizeof(lib.GvCommandLayout) == 28
    for method in ("bind_geometry", "set_command_layout", "emit_draw_commands", "draw_commands_device", "draw_commands"):
        assert callable(getattr(lib.GpuVisibility, method)), method
    if os.path.exists(lib.LIB_PATH):
        handle = lib.load()
        assert handle.gv_abi_version() == 4
        for name, (_, argtypes) in signatures().items():
            fn = getattr(handle, name)
            assert list(fn.argtypes) == argtypes, name
            assert fn.restype in (C.c_int, C.c_int32), name


def test_header_compiles_as_c99_with_the_new_declarations(tmp_path):
    import subprocess
    src = tmp_path / "commands_abi.c"
    src.write_text('#include <stdio.h>\n#include "garden_vis.h"\n'
                   "int main(void) {\n"
                   "    int (*bind)(GvCtx*, uint32_t, const void*, uint32_t, uint32_t, uint32_t, const GvGeometry*, uint32_t) = gv_pool_bind_geometry;\n"
                   "    int (*layout)(GvCtx*, uint32_t, const GvCommandLayout*) = gv_pool_set_command_layout;\n"
                   "    int (*emit)(GvCtx*, uint32_t, uint32_t, uint32_t, void*, size_t) = gv_pool_emit_draw_commands;\n"
                   "    int (*dev)(GvCtx*, uint32_t, const void**, const void**) = gv_pool_draw_commands_device;\n"
                   "    int (*fetch)(GvCtx*, uint32_t, void*, size_t, uint32_t*, uint32_t) = gv_pool_draw_commands_fetch;\n"
                   "    GvGeometry g = {36u, 0u, -4};\n"
                   "    GvCommandLayout l = {20u, 0u, 4u, 8u, 16u, 12u, GV_NONE};\n"
                   '    printf("%u %u %d %u %d %d\\n", (unsigned)GV_MAX_GEOMETRIES, (unsigned)GV_COMMANDS_MERGE_RUNS, (int)GV_DIRTY_GEOMETRY,\n'
                   "           l.stride + g.count, (int)g.vertex_offset, bind && layout && emit && dev && fetch);\n"
                   "    return 0;\n}\n")
    obj = tmp_path / "commands_abi.o"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(obj)], check=True)


# ---- the restatement against answers written out by hand ------------------------------------------------------------------------

def fetched_of(*views):
    return [dict(draw_count=len(v), visible_idx=np.array(v, np.uint32)) for v in views]


def test_restatement_per_draw_known_answer():
    """five draws of one view after an emission of one instance per draw (starts 0, 5); id 9 is outside the 3-entry table"""
    table = csup.geometry_table([(6, 0, 0), (36, 6, 4), (12, 42, -3)])
    ids = np.array([1, 0, 2, 1, 9], np.uint32)  # per POOL slot
    got, counts = csup.expected(fetched_of([4, 2, 0, 3, 1]), [0, 5], None, ids, table, csup.INDEXED, pattern=csup.background(6, 20))
    want = b"".join([struct.pack("<IIIiI", 0, 0, 0, 0, 0),      # slot 4, id 9: the void command, no instance
                     struct.pack("<IIIiI", 12, 1, 42, -3, 1),   # slot 2, id 2
                     struct.pack("<IIIiI", 36, 1, 6, 4, 2),     # slot 0, id 1
                     struct.pack("<IIIiI", 36, 1, 6, 4, 3),     # slot 3, id 1 (not merged: per-draw mode)
                     struct.pack("<IIIiI", 6, 1, 0, 0, 4),      # slot 1, id 0
                     b"\xa5" * 20])                             # behind the last command: untouched
    assert got.tobytes() == want and counts.tolist() == [5]


def test_restatement_run_known_answer():
    """ids 3 3 7 7 7 3 with counts 1 2 0 1 1 4 after a draw emission: three runs, a zero-count draw inside the second"""
    rows = [(0, 0, 0)] * 8
    rows[3], rows[7] = (30, 300, 3), (70, 700, -7)
    first_instance, draw_starts, starts = [0, 1, 3, 3, 4, 5, 9], [0, 6], [0, 9]
    ids = np.array([3, 3, 7, 7, 7, 3], np.uint32)
    got, counts = csup.expected(fetched_of([0, 1, 2, 3, 4, 5]), starts, (first_instance, draw_starts), ids, csup.geometry_table(rows), csup.GAPS,
                                merge=True, pattern=csup.background(4, 32))
    # GAPS: words (gap, instance_count, count, draw, vertex_offset, first, gap, first_instance)
    want = b"".join([struct.pack("<IIIIiIII", 0, 3, 30, 0, 3, 300, 0, 0),    # draws 0, 1: instances 0 .. 2
                     struct.pack("<IIIIiIII", 0, 2, 70, 2, -7, 700, 0, 3),   # draws 2, 3, 4: instances 3, 4 (draw 2 takes none)
                     struct.pack("<IIIIiIII", 0, 4, 30, 5, 3, 300, 0, 5),    # draw 5: instances 5 .. 8; id 3 again, a run of its own
                     b"\xa5" * 32])
    assert got.tobytes() == want and counts.tolist() == [3]
    per_draw, counts = csup.expected(fetched_of([0, 1, 2, 3, 4, 5]), starts, (first_instance, draw_starts), ids, csup.geometry_table(rows),
                                     csup.GAPS, pattern=csup.background(6, 32))
    assert per_draw.view(csup.GAPS)["instance_count"].reshape(-1).tolist() == [1, 2, 0, 1, 1, 4] and counts.tolist() == [6]


def test_restatement_region_known_answer():
    """two views in regions of 2: view 0 has three draws (the third is cut, its count stays true), view 1 has one (one all-zero
    padding command); a target of 3 positions leaves the padding position unwritten too"""
    table = csup.geometry_table([(6, 0, 0), (9, 6, 1)])
    ids = np.array([0, 1, 0], np.uint32)
    fetched = fetched_of([0, 1, 2], [2])
    got, counts = csup.expected(fetched, [0, 3, 4], None, ids, table, csup.PLAIN, region=2, pattern=csup.background(5, 16))
    want = b"".join([struct.pack("<IIII", 6, 1, 0, 0), struct.pack("<IIII", 9, 1, 6, 1),  # view 0: draws 0, 1
                     struct.pack("<IIII", 6, 1, 0, 3), b"\x00" * 16,                      # view 1: draw 0, padding
                     b"\xa5" * 16])
    assert got.tobytes() == want and counts.tolist() == [3, 1]
    cut, counts = csup.expected(fetched, [0, 3, 4], None, ids, table, csup.PLAIN, region=2, capacity=3, pattern=csup.background(5, 16))
    assert cut.tobytes() == want[:48] + b"\xa5" * 32 and counts.tolist() == [3, 1]
