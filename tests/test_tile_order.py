"""The dispatch orders of the linear-scan cull (garden_amd/csrc/gv_tile_order.hpp: the identity and the XCD runs) as conditions on
the header's own text, compiled with gcc into a ctypes twin: under every order launch_cull can choose for S units, the workgroups
of grid_for_tiles() take every unit of [0, S) exactly once, every other workgroup is told to leave (its unit is >= S), and there
are fewer of those than tile_order_surplus_bound() states. The rule that gives a Hi-Z view fewer tiles per workgroup
(hot_tiles_per_workgroup_hiz in gv_kernels.hpp) is read from its text."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hiz_paths_support import header_constant, source_text

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "garden_amd", "csrc")

_TWIN_SRC = r"""
#include <string.h>
#include "gv_tile_order.hpp"
/* 0 when `order` over `units` units meets the conditions; seen: `units` bytes of scratch */
int twin_check(uint32_t units, uint32_t order, uint8_t* seen)
{
    const uint32_t grid = grid_for_tiles(units, order);
    uint32_t left = 0, b, u;
    if (grid < units)
        return 1;
    if (grid - units >= tile_order_surplus_bound(order))
        return 2;
    memset(seen, 0, units);
    for (b = 0; b < grid; b++) {
        u = tile_of_workgroup(b, order);
        if (u >= units) {
            left++;
            continue;
        }
        if (seen[u])
            return 3;
        seen[u] = 1;
    }
    for (u = 0; u < units; u++)
        if (!seen[u])
            return 4;
    return left == grid - units ? 0 : 5;
}
uint32_t twin_xcd_run(uint32_t tiles) { return xcd_run_for_tiles(tiles); }
uint32_t twin_grid(uint32_t units, uint32_t order) { return grid_for_tiles(units, order); }
uint32_t twin_unit(uint32_t b, uint32_t order) { return tile_of_workgroup(b, order); }
"""

SIZES = list(range(1, 4101)) + [8192, 8193, 9766, 16384, 39063, 2 ** 20 + 1]


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_order")
    src, out = os.path.join(str(d), "tile_order_twin.c"), os.path.join(str(d), "libtile_order_twin.so")
    with open(src, "w") as f:
        f.write(_TWIN_SRC)
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, src, "-o", out], check=True)
    lib = C.CDLL(out)
    u32 = C.c_uint32
    lib.twin_check.argtypes, lib.twin_check.restype = [u32, u32, C.c_void_p], C.c_int
    for name, n in (("twin_xcd_run", 1), ("twin_grid", 2), ("twin_unit", 2)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [u32] * n, u32
    return lib


def hot_tiles(tiles, hiz):
    """launch_cull's tiles per workgroup for a sphere-stream pool of `tiles` tiles, restated from gv_kernels.hpp"""
    k4, k2 = HOT_STEPS
    k = 4 if tiles >= k4 else (2 if tiles >= k2 else 1)
    if hiz and k > 1:
        k = 4 if tiles >= HIZ_K4 else (2 if tiles >= HIZ_K2 else 1)
    return k


_M = re.search(r"return tiles >= (\d+)u \? 4u : \(tiles >= (\d+)u \? 2u : 1u\);", source_text("gv_kernels.hpp"))
HOT_STEPS = (int(_M.group(1)), int(_M.group(2)))
HIZ_K2, HIZ_K4 = header_constant("gv_kernels.hpp", "kHizHotK2Tiles"), header_constant("gv_kernels.hpp", "kHizHotK4Tiles")


def orders_for(lib, units):
    """every order launch_cull can hand a kernel for `units` units: the identity (Hi-Z views), the frustum-only views' XCD runs for
    tiles, and for super-tiles of 2 and 4 the run of the pool's tiles divided by K (the last super-tile full or holding one tile)"""
    out = {0, lib.twin_xcd_run(units)}
    for k in (2, 4):
        for tiles in (units * k, units * k - (k - 1)):
            out.add(lib.twin_xcd_run(tiles) // k)
    return sorted(out)


def test_every_order_takes_every_unit_exactly_once(twin):
    seen = np.zeros(max(SIZES), dtype=np.uint8)
    runs = 0
    for units in SIZES:
        for order in orders_for(twin, units):
            assert twin.twin_check(units, order, seen.ctypes.data) == 0, (units, order)
            runs += order != 0
    assert runs  # the XCD runs are chosen for some of these sizes


def test_an_xcd_streams_its_runs(twin):
    tiles = 39063  # the bench pool
    run = twin.twin_xcd_run(tiles)
    assert run == 256
    for q in (0, 1, 5):
        for xcd in range(8):
            first = twin.twin_unit((q * run) * 8 + xcd, run)
            assert first == (8 * q + xcd) * run
            assert [twin.twin_unit((q * run + j) * 8 + xcd, run) for j in (1, 2, run - 1)] == [first + 1, first + 2, first + run - 1]


def test_frustum_only_views_keep_their_xcd_runs_and_hiz_views_the_identity(twin):
    assert [twin.twin_xcd_run(t) for t in (1, 2047, 2048, 16383, 16384, 39063)] == [0, 0, 32, 32, 256, 256]
    text = source_text("gv_cull.hip")
    assert "a.xcd_run = vp.use_hiz ? 0 : xcd_run_for_tiles(a.nblocks);" in text
    assert "a.xcd_run = vp.use_hiz ? 0 : xcd_run_for_tiles(a.nblocks) / tiles_each;" in text
    # the kernels, the launch and this test read one text
    assert '#include "gv_tile_order.hpp"' in source_text("gv_device.hpp")
    assert text.count("tile_of_workgroup(blockIdx.x, args.xcd_run)") == 2


def test_a_hiz_view_takes_no_more_tiles_per_workgroup_than_a_frustum_only_view():
    assert "const uint32_t tiles_each = vp.use_hiz && k > 1 ? hot_tiles_per_workgroup_hiz(a.nblocks) : k;" in source_text("gv_cull.hip")
    assert HOT_STEPS[1] <= HIZ_K2 <= HIZ_K4 and HOT_STEPS[0] <= HIZ_K4
    for tiles in SIZES + [HIZ_K2 - 1, HIZ_K2, HIZ_K4 - 1, HIZ_K4, 78125]:
        k, kh = hot_tiles(tiles, False), hot_tiles(tiles, True)
        assert kh <= k and 16 % kh == 0  # a super-tile never straddles an emit chunk of 16 tiles
    assert [hot_tiles(t, True) for t in (8192, 16383, 16384, 39063, 54688, 65537)] == [1, 1, 2, 2, 2, 4]
    assert [hot_tiles(t, False) for t in (8191, 8192, 16383, 16384, 39063)] == [1, 2, 2, 4, 4]
