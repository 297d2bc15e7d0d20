"""gv_pool_group_draws on the CPU tier: the header declares the entry point with the signature garden_amd/lib.py binds, the library
exports it, GV_GROUP_BY_LOD is there, the ABI version is still 4 (the change is additive) — and a census of the GPU case table
(tests/group_support.py): its tile and block constants are the kernel header's, it holds the counts and key widths at which the
kernels change path, and every case's CPU restatement meets the conditions that keep it from passing by accident."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import group_support as gsup
import lod_support as lsup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, U32, F32 = C.c_void_p, C.c_uint32, C.c_float
NAME = "gv_pool_group_draws"
PARAMS = "GvCtx* ctx, uint32_t pool_id, uint32_t view_index, uint32_t flags, float view_scale"
ARGTYPES = [P, U32, U32, U32, F32]


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "garden_vis.h")).read(), flags=re.S)


def test_header_declares_the_entry_point_with_this_signature():
    text = header()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, text)
    assert m, NAME
    assert " ".join(m.group(1).split()) == PARAMS
    assert re.search(r"#define GV_GROUP_BY_LOD 1u?\b", text)
    assert re.search(r"#define GV_ABI_VERSION 4u?\b", text)


def test_library_exports_it_and_lib_py_binds_the_same_signature():
    from garden_amd import lib
    assert NAME in lib.EXPORTS
    assert lib.GV_GROUP_BY_LOD == 1
    assert callable(lib.GpuVisibility.group_draws)
    if os.path.exists(lib.LIB_PATH):
        handle = lib.load()
        assert handle.gv_abi_version() == 4
        fn = getattr(handle, NAME)
        assert list(fn.argtypes) == ARGTYPES
        assert fn.restype in (C.c_int, C.c_int32)


def test_header_compiles_as_c99_with_the_new_declaration(tmp_path):
    src = tmp_path / "group_abi.c"
    src.write_text('#include <stdio.h>\n#include "garden_vis.h"\n'
                   "int main(void) {\n"
                   "    int (*group)(GvCtx*, uint32_t, uint32_t, uint32_t, float) = gv_pool_group_draws;\n"
                   '    printf("%u %d\\n", (unsigned)GV_GROUP_BY_LOD, group != 0);\n'
                   "    return 0;\n}\n")
    obj = tmp_path / "group_abi.o"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(obj)], check=True)


# ---- the census of the GPU case table ---------------------------------------------------------------------------------------------

def test_case_table_is_built_around_the_kernel_headers_constants():
    assert gsup.header_constants() == gsup.HEADER_NAMES
    from delivery_support import BATCH_SORT_MAX, MID_SORT_MAX, PUBLISH_MAX
    assert (gsup.BATCH_SORT_MAX, gsup.PUBLISH_MAX) == (BATCH_SORT_MAX, PUBLISH_MAX) and gsup.SORT_AT_ONCE == MID_SORT_MAX + 3
    assert gsup.TILE % gsup.BLOCK == 0 and gsup.TILE <= 65536  # 16-bit ranks


def test_case_table_holds_every_count_and_key_width_at_which_the_kernels_change_path():
    counts = {c.n for c in gsup.CASES}
    T = gsup.TILE
    for n in (1, 2, 255, 256, 257, T - 1, T, T + 1, 16384, 16385, 40000, 300000, (1 << 20) + 3):
        assert n in counts, n
    assert 300000 > gsup.PUBLISH_MAX
    assert any(c.n > T * gsup.GROUP_TILES for c in gsup.CASES)  # more than one group of tiles
    tables = {c.K for c in gsup.CASES if not c.by_lod}
    assert {1, 200, 256, 257, 65535, 65536} <= tables
    assert [gsup.digits(k) for k in (1, 200, 255, 256, 257, 65535, 65536)] == [1, 1, 1, 2, 2, 2, 3]
    assert {c.width for c in gsup.CASES} == {None, 1, 2, 4}
    assert {c.presort for c in gsup.CASES if c.n in (16384, (1 << 20) + 3)} == {False, True}
    assert any(c.by_lod and c.width is None for c in gsup.CASES) and any(c.by_lod and c.width for c in gsup.CASES)
    assert len({c.name for c in gsup.CASES}) == len(gsup.CASES)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return lsup.build_twin(tmp_path_factory.mktemp("lod_twin"))


@pytest.mark.parametrize("case", gsup.CASES, ids=lambda c: c.name)
def test_every_case_meets_the_conditions_on_its_cpu_restatement(case, twin):
    """the ids of the case's world under a stand-in delivery order (gsup.stand_in_order): not grouped already, not the identity,
    several members per key where the keys are few; and the planted ids are where the table says"""
    c = case
    order = gsup.stand_in_order(c.n)
    if c.by_lod:
        from garden_amd import scene
        positions = scene.flat_scene(c.n, defects=False).transforms["position"]
        w = gsup.LodWorld(positions)
        models = np.stack([lsup.model_at(*positions[s][:3]) for s in order])
        ids = w.ids if c.width else None
        kappa = gsup.keys(order, ids, c.K, lod=(twin, models, w.sizes, 1.0, w.lod))
        plain = gsup.keys(order, ids, c.K)
        assert kappa.tolist() != plain.tolist()  # the levels take part in the keys
        assert len(np.unique(kappa)) == (w.levels if ids is None else w.levels * w.bases)
    else:
        ids = gsup.case_ids(c)
        kappa = gsup.keys(order, ids, c.K)
        if c.n >= 256:
            for special in gsup.SPECIAL_IDS:
                if special <= np.iinfo(ids.dtype).max:
                    assert np.count_nonzero(ids == special) >= 3, special
        assert int(kappa.max()) <= c.K
        if c.n >= 256 and int(ids.max()) >= c.K:
            assert np.count_nonzero(kappa == c.K) >= 3  # the void bucket is in use
    gsup.check_conditions(kappa, order)
    # the restatement itself: grouped, stable
    pi = gsup.order_of(kappa)
    assert (np.diff(kappa[pi].astype(np.int64)) >= 0).all()
    same = np.diff(kappa[pi].astype(np.int64)) == 0
    assert (np.diff(pi)[same] > 0).all()
