"""gv_pool_select_lods and its companions on the CPU tier: the header declares the entry points with the signatures garden_amd/lib.py
binds, the library exports them, the new constants are there, the ABI version is still 4 (the change is additive), and the C twin
of the rule the GPU tests compare against (tests/lod_twin.h) gives the known answers written out by hand below."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lod_support as lsup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P, U32, F32 = C.c_void_p, C.c_uint32, C.c_float


def signatures():
    from garden_amd import lib
    # name -> (the parameter list of the header, whitespace squeezed; the argtypes lib.py must bind)
    return {
        "gv_pool_bind_lod": (
            "GvCtx* ctx, uint32_t pool_id, const void* sizes, uint32_t stride, uint32_t occupancy, const GvLodGeometry* table, "
            "uint32_t table_count", [P, U32, P, U32, U32, C.POINTER(lib.GvLodGeometry), U32]),
        "gv_pool_select_lods": ("GvCtx* ctx, uint32_t pool_id, const float* view_scale, uint32_t view_count", [P, U32, C.POINTER(F32), U32]),
        "gv_pool_lods_device": ("GvCtx* ctx, uint32_t pool_id, const void** draw_geometry, const void** level_counts",
                                [P, U32, C.POINTER(P), C.POINTER(P)]),
        "gv_pool_lods_fetch": (
            "GvCtx* ctx, uint32_t pool_id, uint32_t* draw_geometry, uint32_t capacity, uint32_t* level_counts, uint32_t counts_capacity",
            [P, U32, C.POINTER(U32), U32, C.POINTER(U32), U32]),
    }


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "garden_vis.h")).read(), flags=re.S)


def test_header_declares_the_entry_points_with_these_signatures():
    text = header()
    for name, (params, _) in signatures().items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        assert " ".join(m.group(1).split()) == params, name
    assert re.search(r"#define GV_MAX_LOD_LEVELS 8u?\b", text)
    assert re.search(r"\bGV_DIRTY_LOD = 5\b", text)
    assert re.search(r"#define GV_ABI_VERSION 4u?\b", text)


def test_library_exports_them_and_lib_py_binds_the_same_signatures():
    from garden_amd import lib
    for name in signatures():
        assert name in lib.EXPORTS, name
    assert lib.GV_MAX_LOD_LEVELS == 8 and lib.GV_DIRTY_LOD == 5
    assert C.sizeof(lib.GvLodGeometry) == 32 and lib.LOD_DTYPE.itemsize == 32 and lib.LOD_DTYPE == lsup.LOD_DTYPE
    for method in ("bind_lod", "select_lods", "lods", "lods_device"):
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
    src = tmp_path / "lod_abi.c"
    src.write_text('#include <stdio.h>\n#include "garden_vis.h"\n'
                   "typedef char lod_geometry_is_32_bytes[sizeof(GvLodGeometry) == 32 ? 1 : -1];\n"
                   "int main(void) {\n"
                   "    int (*bind)(GvCtx*, uint32_t, const void*, uint32_t, uint32_t, const GvLodGeometry*, uint32_t) = gv_pool_bind_lod;\n"
                   "    int (*select)(GvCtx*, uint32_t, const float*, uint32_t) = gv_pool_select_lods;\n"
                   "    int (*dev)(GvCtx*, uint32_t, const void**, const void**) = gv_pool_lods_device;\n"
                   "    int (*fetch)(GvCtx*, uint32_t, uint32_t*, uint32_t, uint32_t*, uint32_t) = gv_pool_lods_fetch;\n"
                   "    GvLodGeometry g = {4u, {10.0f, 20.0f, 40.0f, 0.0f, 0.0f, 0.0f, 0.0f}};\n"
                   '    printf("%u %d %u %d\\n", (unsigned)GV_MAX_LOD_LEVELS, (int)GV_DIRTY_LOD, g.levels + (unsigned)g.switch_at[2],\n'
                   "           bind && select && dev && fetch);\n"
                   "    return 0;\n}\n")
    obj = tmp_path / "lod_abi.o"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(obj)], check=True)


# ---- the twin against answers written out by hand -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return lsup.build_twin(tmp_path_factory.mktemp("lod_twin"))


ONE_ULP_UP = np.nextafter(np.float32(1.0), np.float32(2.0))
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def test_twin_tie_keeps_the_finer_level_and_one_ulp_switches(twin):
    """pivot (3, 4, 0): d2 = 25 exactly; size 1, threshold 5: q = 25 — x > q is false. With the scale one ulp above 1, x is the float
    above 25 and the draw switches."""
    assert lsup.twin_level(twin, lsup.model_at(3, 4, 0), 1.0, 1.0, 2, [5.0]) == 0
    assert lsup.twin_level(twin, lsup.model_at(3, 4, 0), 1.0, ONE_ULP_UP, 2, [5.0]) == 1
    assert lsup.twin_level(twin, lsup.model_at(0, -3, 4), 2.0, 1.0, 2, [2.5]) == 0  # (the order of the terms: 0, 9, 16 -> 25; 2 x 2.5 = 5)


def test_twin_nan_gives_the_finest_and_inf_the_coarsest(twin):
    sw = [1.0, 2.0, 3.0, 4.0, 5.0]
    assert lsup.twin_level(twin, lsup.model_at(100, 0, 0), NAN, 1.0, 6, sw) == 0            # a NaN size: every q is NaN
    assert lsup.twin_level(twin, lsup.model_at(NAN, 0, 0), 1.0, 1.0, 6, sw) == 0            # a NaN distance
    assert lsup.twin_level(twin, lsup.model_at(100, 0, 0), 1.0, NAN, 6, sw) == 0            # a NaN scale
    assert lsup.twin_level(twin, lsup.model_at(INF, 0, 0), 1.0, 1.0, 6, sw) == 5            # +inf distance: levels - 1
    assert lsup.twin_level(twin, lsup.model_at(3e19, 3e19, 0), 1.0, 1.0, 6, sw) == 5        # d2 overflows to +inf
    assert lsup.twin_level(twin, lsup.model_at(INF, 0, 0), 1.0, 0.0, 6, sw) == 0            # inf x 0 = NaN
    assert lsup.twin_level(twin, lsup.model_at(100, 0, 0), INF, 1.0, 6, sw) == 0            # an infinite size: every q is +inf
    assert lsup.twin_level(twin, lsup.model_at(INF, 0, 0), 1.0, 1.0, 3, [1.0, INF]) == 1    # inf > inf is false


def test_twin_counts_unsorted_thresholds(twin):
    """distance 6 over thresholds 10, 1, 5: x = 36 exceeds q = 1 and 25, not 100 — level 2; a search for the first threshold not
    exceeded would answer 0"""
    assert lsup.twin_level(twin, lsup.model_at(0, 0, 6), 1.0, 1.0, 4, [10.0, 1.0, 5.0]) == 2
    assert lsup.twin_level(twin, lsup.model_at(0, 0, 6), 1.0, 1.0, 3, [10.0, 1.0, 5.0]) == 1  # only levels - 1 thresholds are read


def test_twin_one_level_and_ids_outside_the_table(twin):
    assert lsup.twin_level(twin, lsup.model_at(1e6, 0, 0), 1.0, 1.0, 1, [0.0] * 7) == 0     # levels == 1
    table = lsup.lod_table([(4, [1.0, 2.0, 3.0]), (1, []), (8, [1, 2, 3, 4, 5, 6, 7])])
    models = np.stack([lsup.model_at(0, 0, 100)] * 6)
    base = np.array([0, 1, 2, 3, 70000, 0xFFFFFFFF], np.uint32)  # 3 = lod_table_count: one level
    g, hist = lsup.twin_many(twin, models, base, np.ones(6, np.float32), 1.0, table)
    assert g.tolist() == [3, 1, 9, 3, 70000, 0xFFFFFFFF]
    assert hist.tolist() == [4, 0, 0, 1, 0, 0, 0, 1]


def test_twin_add_wraps(twin):
    assert twin.twin_effective(0xFFFFFFFF, 1) == 0 and twin.twin_effective(0xFFFFFFFE, 7) == 5
    assert twin.twin_effective(8, 3) == 11


def test_command_restatement_takes_per_draw_ids():
    """two views of the same three slots at different levels: the per-draw ids decide, not the slots"""
    import struct
    import commands_support as csup
    table = csup.geometry_table([(6, 0, 0), (9, 6, 1), (12, 15, 2)])
    fetched = [dict(draw_count=3, visible_idx=np.array([2, 0, 1], np.uint32)), dict(draw_count=2, visible_idx=np.array([0, 2], np.uint32))]
    got, counts = lsup.expected_commands(fetched, [0, 3, 5], None, [[0, 0, 1], [2, 7]], table, csup.PLAIN, merge=True,
                                         pattern=csup.background(5, 16))
    want = b"".join([struct.pack("<IIII", 6, 2, 0, 0), struct.pack("<IIII", 9, 1, 6, 2),   # view 0: a run of two, one draw
                     struct.pack("<IIII", 12, 1, 15, 3), struct.pack("<IIII", 0, 0, 0, 4),  # view 1: level 2, then the void command
                     b"\xa5" * 16])
    assert got.tobytes() == want and counts.tolist() == [2, 2]
