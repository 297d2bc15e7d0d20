"""CPU tier of the pyramid slots: the two calls and GV_MAX_PYRAMIDS agree between include/garden_vis.h, the library's exports and
the ctypes binding; GvView keeps its size; and the census of tests/pyramid_slots_support.py::CASES on the ORACLE alone — conditions
on the inputs, not measurements: they keep tests/test_gpu_pyramid_slots.py from passing by accident (an image that hides nothing,
or everything, or two pyramids that could be exchanged unnoticed)."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import pyramid_slots_support as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENSUS_MIN_ENTITIES = 257  # the share census: the issue's own bound (smaller pools show a view a handful of entities at most)
EXCHANGE_MIN_ENTITIES = 2  # the exchange census: every case but the pool of ONE entity, whose views hold it or nothing — no two
                           # pyramids can be told apart by a set of at most one element that the frustum alone decides


def header_text():
    return open(os.path.join(ROOT, "include", "garden_vis.h")).read()


def test_header_exports_and_binding_agree_on_the_two_calls():
    from garden_amd import lib
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    assert re.search(r"\bint\s+gv_hiz_select\s*\(\s*GvCtx\s*\*\s*ctx\s*,\s*uint32_t\s+pyramid\s*\)\s*;", text)
    assert re.search(r"\bint\s+gv_hiz_drop\s*\(\s*GvCtx\s*\*\s*ctx\s*,\s*uint32_t\s+pyramid\s*\)\s*;", text)
    handle = lib.load()
    for name in ("gv_hiz_select", "gv_hiz_drop"):
        assert name in lib.EXPORTS and hasattr(handle, name), name
        assert getattr(handle, name).argtypes == [ctypes.c_void_p, ctypes.c_uint32], name
    assert hasattr(lib.GpuVisibility, "hiz_select") and hasattr(lib.GpuVisibility, "hiz_drop")
    assert handle.gv_abi_version() == 4  # additive: the version stays


def test_max_pyramids_is_one_per_view():
    from garden_amd import lib
    m = re.search(r"#define\s+GV_MAX_PYRAMIDS\s+(\d+)u", header_text())
    assert m and int(m.group(1)) == lib.GV_MAX_PYRAMIDS == lib.GV_MAX_VIEWS == 8
    assert lib.GV_MAX_PYRAMIDS + 1 <= 255  # use_hiz is a byte: 1 + k fits


def test_a_null_context_is_an_argument_error_without_a_device():
    from garden_amd import lib
    handle = lib.load()
    assert handle.gv_hiz_select(None, 0) == lib.GV_E_ARG and handle.gv_hiz_drop(None, 0) == lib.GV_E_ARG


def test_view_and_config_keep_their_sizes(tmp_path):
    import subprocess
    from garden_amd import lib
    assert ctypes.sizeof(lib.GvView) == 16 * 4 + 4 * 4 + 4 * 4 + 4 and ctypes.sizeof(lib.GvConfig) == 16  # as tests/test_abi.py pins them
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "garden_vis.h"\nint main(void) { printf("%zu %zu %zu %u\\n", sizeof(GvView), '
                   'sizeof(GvConfig), offsetof(GvView, use_hiz), (unsigned)GV_MAX_PYRAMIDS); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [ctypes.sizeof(lib.GvView), 16, lib.GvView.use_hiz.offset, 8]


def test_the_case_table_is_what_the_issue_asks_for():
    sizes = {c.n for c in ps.CASES}
    assert {1, 64, 65, 257, 4097, 20_011, 70_007} <= sizes
    assert any(c.n == 70_007 and c.fixture == "gpu_bounds" for c in ps.CASES)
    assert {c.MAP for c in ps.CASES} == {"exact", "speculate", "general"} and any(c.depth == 3 for c in ps.CASES)
    assert {"gpu", "gpu_slot_order", "gpu_bounds", "rg16f"} == {c.fixture for c in ps.CASES}
    used = {s for c in ps.CASES for s in c.sets}
    assert used == set(ps.VIEW_SETS)
    bytes_of = {ps.VIEW_SETS[s].use_hiz for s in used}
    assert {(1, 2), (0, 2, 3, 4), (2, 2, 3), (3, 0, 1), tuple(range(1, 9))} <= bytes_of
    assert any(set(ps.VIEW_SETS[s].emit) == {0, 1} for s in used)
    assert any(ps.VIEW_SETS[s].kinds[0] == "main" and "main" not in ps.VIEW_SETS[s].kinds[1:] for s in used)
    # every image size is some pyramid's, in both texel formats
    for rg16f in (False, True):
        seen = {ps.image_size(c, k) for c in ps.CASES if (c.fixture == "rg16f") == rg16f for k in ps.pyramids_of(c)}
        assert seen == set(ps.IMAGE_SIZES), (rg16f, seen)
    # non-exact mappings are what the slot-order mirror gives a shuffled pool; pools that pair slot for slot are exact anywhere
    import cull_paths_support as cp
    for c in ps.CASES:
        if ps.FIXTURE_FLAGS[c.fixture].slot_order:
            assert cp.mirror_mapping(ps.build_scene(c)) == c.MAP, c.name
        else:
            assert c.MAP == "exact", c.name


def test_every_reachable_instantiation_of_the_new_kernel_has_a_case():
    """cull_multi_hiz_kernel<MAP, BOUNDS> x {view 0 queries or not}: all twelve are reachable (block bounds by flag for exact pools,
    by size for any mapping)"""
    cells = {ps.kernel_cell(c, s) for c in ps.CASES for s in c.sets if ps.takes_new_form(s)}
    assert cells == set(itertools.product(("exact", "speculate", "general"), (False, True), (False, True))), cells
    assert all(ps.takes_new_form(s) for s in ps.VIEW_SETS)  # (no set of the table falls back to the old plan)


@pytest.mark.parametrize("c", [c for c in ps.CASES if c.n >= EXCHANGE_MIN_ENTITIES], ids=lambda c: c.name)
def test_census_of_the_depth_images_on_the_oracle(oracle, c):
    """Per Hi-Z view: the view's own pyramid drops at least 5 % and keeps at least 5 % of its frustum survivors. Per two views of a
    set that name different pyramids: exchanging the two pyramids changes BOTH visible sets — a kernel that wires pyramid j to view i
    cannot pass. (The first holds from 257 entities on, the issue's own bound; the second for every case but the pool of one entity.)"""
    sc = ps.build_scene(c)
    rg16f = c.fixture == "rg16f"
    pyramids = {k: ps.oracle_pyramid(oracle, c, k, rg16f) for k in ps.pyramids_of(c)}

    def visible(view, hz):
        out = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, view, hiz=hz, threads=4)
        return np.sort(out["visible_idx"][:out["draw_count"]])

    for s in c.sets:
        views = ps.make_views(c, s)
        own = {}
        for i, v in enumerate(views):
            if not v["use_hiz"]:
                continue
            k = ps.pyramid_of(v["use_hiz"])
            survivors = visible(dict(v, use_hiz=0), None).size
            own[i] = visible(v, pyramids[k])
            kept = own[i].size
            print(f"{c.name} {s} view {i} pyramid {k} {ps.image_size(c, k)}: {survivors} in the frustum, {kept} kept")
            if c.n >= CENSUS_MIN_ENTITIES:
                assert survivors - kept >= 0.05 * survivors and kept >= 0.05 * survivors, (c.name, s, i, survivors, kept)
        for i, j in itertools.combinations(own, 2):
            ki, kj = ps.pyramid_of(views[i]["use_hiz"]), ps.pyramid_of(views[j]["use_hiz"])
            if ki == kj:
                continue
            assert not np.array_equal(visible(views[i], pyramids[kj]), own[i]), (c.name, s, i, j)
            assert not np.array_equal(visible(views[j], pyramids[ki]), own[j]), (c.name, s, i, j)
