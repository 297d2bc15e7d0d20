"""gv_pick on the CPU tier: the header declares it and the library exports it, the ctypes mirrors of GvPickRay / GvPickHit match
the C layout, and the C twin of the picking arithmetic (tests/pick_twin.h) passes hand-derived cases."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pick_support as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_gv_pick():
    import re
    from garden_amd import lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "garden_vis.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+gv_pick\s*\(", text)
    assert "gv_pick" in lib.EXPORTS
    handle = lib.load()
    assert hasattr(handle, "gv_pick")
    assert handle.gv_abi_version() == 4
    assert lib.GV_MAX_PICK_RAYS == int(re.search(r"#define GV_MAX_PICK_RAYS (\d+)u", text).group(1))


def test_pick_structs_match_the_header(tmp_path):
    from garden_amd import lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "garden_vis.h"', "int main(void) {"]
    for name in ("GvPickRay", "GvPickHit"):
        lines.append(f'    printf("{name} %zu", sizeof({name}));')
        for field, _ in getattr(lib, name)._fields_:
            lines.append(f'    printf(" %zu", offsetof({name}, {field}));')
        lines.append('    printf("\\n");')
    lines += ["    return 0;", "}"]
    src = tmp_path / "pick_abi.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "pick_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = set()
    for line in filter(None, out):
        name, size, *offsets = line.split()
        cls = getattr(lib, name)
        assert int(size) == ctypes.sizeof(cls), name
        assert [int(o) for o in offsets] == [getattr(cls, f).offset for f, _ in cls._fields_], name
        seen.add(name)
    assert seen == {"GvPickRay", "GvPickHit"}
    assert ctypes.sizeof(lib.GvPickRay) == 32 and ctypes.sizeof(lib.GvPickHit) == 16


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return ps.build_twin(tmp_path_factory.mktemp("twin"))


def model(c0=(1, 0, 0), c1=(0, 1, 0), c2=(0, 0, 1), t=(0, 0, 10)):
    return np.array(list(c0) + list(c1) + list(c2) + list(t), dtype=np.float32)


UNIT = np.array([-1, -1, -1, 1, 1, 1], dtype=np.float32)


def key(twin, m, ray, box=UNIT, order_slot=7):
    m = np.ascontiguousarray(m, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32)
    ray = np.ascontiguousarray(ray, dtype=np.float32)
    return int(twin.twin_key(m.ctypes.data, box.ctypes.data, ray.ctypes.data, order_slot))


def hit_key(dist_sq, order_slot=7):
    return (int(np.float32(dist_sq).view(np.uint32)) << 32) | order_slot


def test_twin_axis_aligned_hit(twin):
    # box [-1, 1]^3 at z = 10 in front of the origin: entered at t = 9; distSq = |o - t|^2 = 100
    assert key(twin, model(), [0, 0, 0, 0, 0, 1]) == hit_key(100.0)
    # the direction is not normalised: same hit with a longer one; the key carries order and slot unchanged
    assert key(twin, model(), [0, 0, 0, 0, 0, 2.5], order_slot=(3 << 28) | 12345) == hit_key(100.0, (3 << 28) | 12345)
    # scale 2 along x: x = 1.5 lies inside the scaled box (model space 0.75)
    assert key(twin, model(c0=(2, 0, 0)), [1.5, 0, 0, 0, 0, 1]) == hit_key(102.25)


def test_twin_near_miss(twin):
    # slope 0.2: |x| <= 1 only for t <= 5, the z slab starts at t = 9
    assert key(twin, model(), [0, 0, 0, 0.2, 0, 1]) == ps.MISS
    # 0.11 reaches x = 0.99 at t = 9: a graze that still enters
    assert key(twin, model(), [0, 0, 0, 0.11, 0, 1]) == hit_key(100.0)
    # 0.112 leaves the x slab at t = 8.93, before the z slab opens
    assert key(twin, model(), [0, 0, 0, 0.112, 0, 1]) == ps.MISS


def test_twin_box_behind_the_origin(twin):
    assert key(twin, model(), [0, 0, 0, 0, 0, -1]) == ps.MISS


def test_twin_origin_inside_the_box(twin):
    # tNear = -1 < 0: a ray that starts inside a box does not pick it (mesh-selector.cpp:106)
    assert key(twin, model(), [0, 0, 10, 0, 0, 1]) == ps.MISS
    assert key(twin, model(), [0.5, 0.5, 9.5, 1, 1, 1]) == ps.MISS


def test_twin_zero_direction_component(twin):
    # d'x == 0: the x slab passes only when min.x <= o'x <= max.x
    assert key(twin, model(), [0.999, 0, 0, 0, 0, 1]) == hit_key(np.float32(0.999) * np.float32(0.999) + np.float32(100.0))
    assert key(twin, model(), [1.001, 0, 0, 0, 0, 1]) == ps.MISS
    assert key(twin, model(), [-1.5, 0, 0, 0, 0, 1]) == ps.MISS
    # on the slab's plane itself: min <= o' <= max holds
    assert key(twin, model(), [1.0, 0, 0, 0, 0, 1]) == hit_key(101.0)
    # a zero direction: every axis passes or fails on position alone, tNear stays -inf: no hit
    assert key(twin, model(), [0, 0, 0, 0, 0, 0]) == ps.MISS


def test_twin_singular_scale(twin):
    # scale.x = 0: det = 0, no inverse, nothing to hit — even for a ray straight through the pivot
    assert key(twin, model(c0=(0, 0, 0)), [0, 0, 0, 0, 0, 1]) == ps.MISS
    # rank-deficient without a zero column
    assert key(twin, model(c0=(1, 1, 0), c1=(1, 1, 0)), [0, 0, 0, 0, 0, 1]) == ps.MISS


def test_twin_nan_and_inf_in_trs(twin):
    nan, inf = float("nan"), float("inf")
    assert key(twin, model(c1=(0, nan, 0)), [0, 0, 0, 0, 0, 1]) == ps.MISS
    assert key(twin, model(t=(0, 0, nan)), [0, 0, 0, 0, 0, 1]) == ps.MISS
    assert key(twin, model(c2=(0, 0, inf)), [0, 0, 0, 0, 0, 1]) == ps.MISS
    # a NaN box never passes a slab
    assert key(twin, model(), [0, 0, 0, 0, 0, 1], box=np.array([-1, -1, nan, 1, 1, 1], np.float32)) == ps.MISS


def test_twin_pool_minimum_and_ties(twin):
    """pick_twin_min: the nearest pivot wins, a tie goes to the lower order and then the lower slot, the excluded slot is skipped"""
    models = np.stack([model(t=(0, 0, 10)), model(t=(0, 0, 20)), model(t=(0, 0, 10))])
    boxes = np.stack([UNIT, UNIT * 5, UNIT])
    pool = ps.Pool([4, 2, 9], models, boxes)
    rays = np.array([[0, 0, 0, 0, 0, 1]], np.float32)
    assert ps.decode(ps.twin_keys(twin, [pool], rays), [0]) == [(0, 4, 100.0)]
    assert ps.decode(ps.twin_keys(twin, [pool], rays, exclude=[4]), [0]) == [(0, 9, 100.0)]
    # the first listed pool keeps the tie even though its slot is the higher one
    assert ps.decode(ps.twin_keys(twin, [pool, pool], rays, exclude=[4, None]), [3, 5]) == [(3, 9, 100.0)]
    assert ps.decode(ps.twin_keys(twin, [pool, pool], rays, exclude=[9, None]), [3, 5]) == [(3, 4, 100.0)]
