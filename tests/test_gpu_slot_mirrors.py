"""The one upload path of the per-slot side columns (upload_slot_mirror in gv_mirror.cpp), once per kind: the payload rows, the ready
counts and the geometry ids. Each case changes its source column everywhere, marks a mix of slots that takes both ways up (three
single slots and a range of 2 047 in the packet, a range of 2 048 as a copy), appends 100 slots (in the packet too), and then compares every emitted
byte with the twin (instances_support) or the restatement of the command rule (commands_support): marked and appended slots show
the new values, unmarked ones the values of the last upload. GvStats.upload_bytes must grow by exactly what the rule gives for the
mix, computed below from the element size.

The marks are the same for every kind: slots 0, 2 998 and 5 999, 2 047 slots from 100, 2 048 slots from 3 000 — the two sides of
kDeviceGatherMinSlots. Marks that touch are merged (DirtyRanges::normalise) and a single slot at 2 999 would travel with the range
behind it, so the middle one sits at 2 998 and every mark reaches the upload as it was made: 2 048 elements go up as one copy,
and 2 150 in the packet — the three single slots, the 2 047, and the 100 appended slots, a range below the threshold like any other.

Where the 100 slots come from differs by kind, as the binding calls do. The payload is rebound with 6 100 rows (same shape: the
mirror stays). The ready counts follow the pool, which is rebound with 6 100 slots. gv_pool_bind_geometry takes every bind as a
new column, so the id mirror has no appended slots: its marks are checked without them, and a rebind with 6 100 ids must upload
all of them."""
import numpy as np
import pytest

import commands_support as csup
import instances_support as isup
from garden_amd import scene
from garden_amd.lib import GV_DIRTY_GEOMETRY, GV_DIRTY_MESH, GV_DIRTY_PAYLOAD, GpuVisibility

pytestmark = pytest.mark.gpu

N, GROWN = 6000, 6100
COPY_MIN = 2048  # kDeviceGatherMinSlots: a range of this many slots or more is copied into its place, smaller ones are packed
MARKS = [(0, 1), (2998, 1), (5999, 1), (100, 2047), (3000, 2048)]  # (disjoint and not touching: none is merged)
SPRITE = isup.layout_dtype(96, mvp=0)  # mvp 0, colour 64, uv 80: the whole stride
SPRITE_AT = [64, 80]


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return isup.build_twin(tmp_path_factory.mktemp("twin"))


@pytest.fixture(scope="module")
def world():
    """6 100 small boxes and the view that holds them all; a case binds the first 6 000 meshes, then all of them"""
    view = scene.make_view(scene.ortho_rev_z(2.0e7, 2.0e7, -1.0e7, 1.0e7), shadow_pass=-1)
    return scene.flat_scene(GROWN, defects=False), view


def bind(vis, sc):
    vis.bind_transforms(sc.transforms, sc.entity_to_transform)
    vis.bind_pool(0, sc.meshes[:N])
    vis.hierarchy_rebuild()


def marked(n):
    mask = np.zeros(n, bool)
    for first, count in MARKS:
        mask[first:first + count] = True
    return mask


def upload_of(elem, mirrored, occupancy, marks=MARKS):
    """upload_bytes of one upload of a column of `elem`-byte elements of which [0, mirrored) are on the device: the marks inside
    the mirrored part, merged where they touch, and the slots behind it; a packed element takes a 4-byte slot word with it"""
    ranges = []
    for lo, hi in sorted((first, min(first + count, mirrored)) for first, count in marks):
        if ranges and lo <= ranges[-1][1]:
            ranges[-1][1] = max(ranges[-1][1], hi)
        elif lo < hi:
            ranges.append([lo, hi])
    if mirrored < occupancy:
        ranges.append([mirrored, occupancy])
    sizes = [hi - lo for lo, hi in ranges]
    copied, packed = sum(s for s in sizes if s >= COPY_MIN), sum(s for s in sizes if s < COPY_MIN)
    return (copied + packed) * elem + packed * 4


def uploaded(vis):
    return vis.stats()["upload_bytes"]


def check_instances(vis, twin, view, occupancy, dtype, fields=(), counts=None):
    """emits view 0 (a draw emission when `counts` is given) and compares every byte of every instance: the twin's mvp of the
    fetched records, the payload `fields` of each record's POOL slot, each record repeated by its slot's count"""
    fetched = vis.fetch(0, write_back=False, occupancy=occupancy, order="raw", pool_id=0)
    assert int(fetched["draw_count"]) == occupancy  # every box is a draw
    exp, _ = isup.expected(twin, dtype, [view], [fetched])
    slots = fetched["visible_idx"].astype(np.int64)
    for field, at in zip(fields, SPRITE_AT):
        raw = np.ascontiguousarray(field).view(np.uint8).reshape(len(field), -1)
        exp[:, at:at + raw.shape[1]] = raw[slots]
    if counts is None:
        vis.emit_instances(0, [0])
    else:
        exp = np.repeat(exp, counts[slots].astype(np.int64), axis=0)
        vis.emit_draw_instances(0, [0])
    got, starts = vis.instances(0)
    assert starts.tolist() == [0, len(exp)]
    assert got.tobytes() == exp.tobytes()


def check_commands(vis, view, occupancy, ids, table):
    """emits view 0's instances and their commands and compares every command byte with the rule over the ids of the POOL slots"""
    fetched = vis.fetch(0, write_back=False, occupancy=occupancy, order="raw", pool_id=0)
    assert int(fetched["draw_count"]) == occupancy
    vis.emit_instances(0, [0])
    pattern = csup.background(occupancy + 7, csup.INDEXED.itemsize)
    exp, counts = csup.expected([fetched], [0, occupancy], None, ids, table, csup.INDEXED, pattern=pattern)
    vis.set_command_layout(0, dtype=csup.INDEXED)
    vis.emit_draw_commands(0)
    host = pattern.copy()
    _, got_counts = vis.draw_commands(0, out=host)
    assert got_counts.tolist() == counts.tolist() == [occupancy]
    assert host.tobytes() == exp.tobytes()


def random_rows(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [rng.integers(0, 1 << 32, (GROWN, 4), dtype=np.uint32) for _ in SPRITE_AT]


# ---- payload rows: elements of `pitch` bytes (two 16-byte fields: 32) ------------------------------------------------------------

def test_payload_rows_marked_and_appended_go_up_the_rest_stays(twin, world):
    sc, view = world
    old, new = random_rows(21), random_rows(22)
    live = [a.copy() for a in old]  # the bound arrays
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_payload(0, [a[:N] for a in live])
        vis.set_instance_layout(0, dtype=SPRITE)
        vis.set_payload_layout(0, SPRITE_AT)
        vis.cull(0, [view])
        check_instances(vis, twin, view, N, SPRITE, old)  # the mirror exists
        for a, b in zip(live, new):
            a[:] = b
        for first, count in MARKS:
            vis.mark_dirty(GV_DIRTY_PAYLOAD, first, count, pool_id=0)
        vis.bind_payload(0, live)  # 6 100 rows of the same shape: 100 appended
        vis.set_payload_layout(0, SPRITE_AT)
        mirrored = [np.where((marked(GROWN) | (np.arange(GROWN) >= N))[:, None], b, a) for a, b in zip(old, new)]
        before = uploaded(vis)
        check_instances(vis, twin, view, N, SPRITE, mirrored)  # the emission uploads: marks made since the cull are seen
        assert uploaded(vis) - before == upload_of(32, N, GROWN)
        vis.bind_pool(0, sc.meshes)  # the pool follows: the appended slots are drawn
        vis.cull(0, [view])  # (its sync appends the pool's own 100 entries)
        before = uploaded(vis)
        check_instances(vis, twin, view, GROWN, SPRITE, mirrored)
        assert uploaded(vis) == before  # no row again


def test_payload_rows_nothing_marked_nothing_travels(twin, world):
    sc, view = world
    rows = random_rows(23)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_payload(0, [a[:N] for a in rows])
        vis.set_instance_layout(0, dtype=SPRITE)
        vis.set_payload_layout(0, SPRITE_AT)
        vis.cull(0, [view])
        check_instances(vis, twin, view, N, SPRITE, rows)
        before = uploaded(vis)
        vis.cull(0, [view])
        check_instances(vis, twin, view, N, SPRITE, rows)
        assert uploaded(vis) == before


# ---- ready counts: 4-byte elements, marked with GV_DIRTY_MESH, appended with the pool -------------------------------------------

def test_ready_counts_marked_and_appended_go_up_the_rest_stays(twin, world):
    sc, view = world
    ready = np.full(GROWN, 2, np.uint32)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ready)
        vis.set_instance_layout(0, dtype=isup.BARE)
        vis.cull(0, [view])
        check_instances(vis, twin, view, N, isup.BARE, counts=ready)  # the mirror exists
        mirrored = np.where(marked(GROWN) | (np.arange(GROWN) >= N), 3, 2).astype(np.uint32)
        ready[:] = 3
        for first, count in MARKS:
            vis.mark_dirty(GV_DIRTY_MESH, first, count, pool_id=0)
        vis.bind_pool(0, sc.meshes)  # 6 100 slots: the column follows the pool, 100 appended
        before = uploaded(vis)
        check_instances(vis, twin, view, N, isup.BARE, counts=mirrored)  # the records are those of the cull; the counts are new
        assert uploaded(vis) - before == upload_of(4, N, GROWN)
        vis.cull(0, [view])  # (its sync settles the pool's own side of the marks and appends its 100 entries)
        before = uploaded(vis)
        check_instances(vis, twin, view, GROWN, isup.BARE, counts=mirrored)
        assert uploaded(vis) == before  # no count again


def test_ready_counts_nothing_marked_nothing_travels(twin, world):
    sc, view = world
    ready = np.full(GROWN, 2, np.uint32)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ready)
        vis.set_instance_layout(0, dtype=isup.BARE)
        vis.cull(0, [view])
        check_instances(vis, twin, view, N, isup.BARE, counts=ready)
        before = uploaded(vis)
        vis.cull(0, [view])
        check_instances(vis, twin, view, N, isup.BARE, counts=ready)
        assert uploaded(vis) == before


# ---- geometry ids: 4-byte elements; every bind is a new column ------------------------------------------------------------------

def geometry_world():
    rng = np.random.Generator(np.random.PCG64(24))
    table = csup.geometry_table([(int(rng.integers(1, 1 << 20)), int(rng.integers(0, 1 << 30)), int(rng.integers(-(1 << 20), 1 << 20)))
                                 for _ in range(8)])
    return rng.integers(0, 4, GROWN, dtype=np.uint32), table


def test_geometry_ids_marked_go_up_the_rest_stays_and_a_rebind_takes_all(world):
    sc, view = world
    old, table = geometry_world()
    ids = old.copy()  # the bound array
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_geometry(0, ids[:N], table)
        vis.set_instance_layout(0, dtype=isup.BARE)
        vis.cull(0, [view])
        check_commands(vis, view, N, old, table)  # the mirror exists
        ids[:] = old + 4  # the other half of the table, everywhere
        for first, count in MARKS:
            vis.mark_dirty(GV_DIRTY_GEOMETRY, first, count, pool_id=0)
        mirrored = np.where(marked(GROWN), ids, old)
        before = uploaded(vis)
        check_commands(vis, view, N, mirrored, table)  # the emission uploads
        assert uploaded(vis) - before == upload_of(4, N, N)
        vis.bind_geometry(0, ids, table)  # 6 100 ids: a new column, marks or not
        before = uploaded(vis)
        check_commands(vis, view, N, ids, table)
        assert uploaded(vis) - before == GROWN * 4
        vis.bind_pool(0, sc.meshes)  # the pool follows: the slots behind 6 000 are drawn
        vis.cull(0, [view])  # (its sync appends the pool's own 100 entries)
        before = uploaded(vis)
        check_commands(vis, view, GROWN, ids, table)
        assert uploaded(vis) == before


def test_geometry_ids_nothing_marked_nothing_travels(world):
    sc, view = world
    ids, table = geometry_world()
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_geometry(0, ids[:N], table)
        vis.set_instance_layout(0, dtype=isup.BARE)
        vis.cull(0, [view])
        check_commands(vis, view, N, ids, table)
        before = uploaded(vis)
        vis.cull(0, [view])
        check_commands(vis, view, N, ids, table)
        assert uploaded(vis) == before
