"""gv_pool_select_lods on the device: the level of detail of every draw of the pool's last instance emission, and the command
emission that takes the selected ids. Expected values come from the C twin of the rule (tests/lod_twin.h) applied to the FETCHED
records, and are exact: every g_k, every level_counts word, and every command byte (tests/lod_support.expected_commands over a 0xA5
background).

The world is a flat pool of N small boxes at random positions, all inside the enclosing main view, so draw_count == N; every case
asserts that, and that visible_idx is not the identity (the mirror's Morton order is in play) — except N == 1. The thresholds are
the world's own quantiles of distance / size, so every level holds about N / levels draws; every case checks that on the CPU
restatement first, so that a kernel which ignores a threshold cannot pass."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import commands_support as csup
import instances_support as isup
import lod_support as lsup
from garden_amd import scene
from garden_amd.lib import (GV_DIRTY_GEOMETRY, GV_DIRTY_LOD, GV_DIRTY_MESH, GV_DIRTY_TRANSFORM, GV_E_ARG, GV_E_STATE,
                            GV_MAX_GEOMETRIES, GV_MAX_LOD_LEVELS, GpuVisibility, GvError, GvLodGeometry)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32P = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return lsup.build_twin(tmp_path_factory.mktemp("lod_twin"))


# ---- the world and helpers of test_gpu_draw_commands.py, re-stated ---------------------------------------------------------------

def enclosing(half=1.0e7, shadow_pass=-1, camera_position=(0, 0, 0), camera_offset=(0, 0, 0)):
    """an orthographic view that holds the whole scene: every box becomes a draw"""
    return scene.make_view(scene.ortho_rev_z(2 * half, 2 * half, -half, half), camera_position=camera_position, camera_offset=camera_offset,
                           shadow_pass=shadow_pass)


def bind(vis, sc, pool_id=0):
    vis.bind_transforms(sc.transforms, sc.entity_to_transform)
    vis.bind_pool(pool_id, sc.meshes)
    vis.hierarchy_rebuild()


def fetch_all(vis, pool_id, listed, occupancy):
    return [vis.fetch(v, write_back=False, occupancy=occupancy, order="raw", pool_id=pool_id) for v in listed]


def whole_world(fetched, n):
    """the case is the size it claims to be, and in the mirror's order"""
    assert int(fetched["draw_count"]) == n
    if n > 1:
        assert fetched["visible_idx"][:n].tolist() != list(range(n))


def instance_starts(vis, pool_id):
    views = vis.instances_info(pool_id)[0]
    starts = np.zeros(views + 1, np.uint32)
    vis._check(vis.lib.gv_pool_instances_fetch(vis.ctx, pool_id, None, 0, starts.ctypes.data_as(U32P), len(starts)))
    return starts


def random_table(count, seed=11):
    rng = np.random.Generator(np.random.PCG64(seed))
    return csup.geometry_table([(int(rng.integers(1, 1 << 20)), int(rng.integers(0, 1 << 30)), int(rng.integers(-(1 << 20), 1 << 20)))
                                for _ in range(count)])


def launches(vis):
    return sum(vis.stats()["launches"].values())


def code(fn, *args, **kw):
    with pytest.raises(GvError) as e:
        fn(*args, **kw)
    return e.value.code


class World:
    """n boxes, `bases` geometries of `levels` levels each: base ids at stride `levels`, the geometry table bases x levels entries"""

    def __init__(self, n, levels=4, bases=7, seed=0):
        self.n, self.levels = n, levels
        self.scene = scene.flat_scene(n, defects=False)
        rng = np.random.Generator(np.random.PCG64(1000 * levels + n + seed))
        self.ids = (rng.integers(0, bases, n) * levels).astype(np.uint32)
        self.sizes = rng.uniform(0.5, 4.0, n).astype(np.float32)
        self.switch_at = lsup.quantile_thresholds(self.scene.transforms["position"], self.sizes, levels)
        # (the entries between the bases are never a base id: one level)
        self.lod = lsup.lod_table([(levels, self.switch_at) if g % levels == 0 else (1, []) for g in range(bases * levels)])
        self.table = random_table(bases * levels)


def balanced(counts, n, levels):
    """the CPU restatement spreads the draws: every level holds at least n / (2 levels) of them"""
    if n >= 256:
        assert (counts[:levels] >= n / (2 * levels)).all(), counts


def select(vis, twin, listed, occupancy, scales, ids, sizes, lod, pool_id=0):
    """Issues the selection behind the pool's last emission and compares every g_k and every level_counts word with the twin over
    the fetched records. Returns (the fetched results, g per view, level_counts)."""
    fetched = fetch_all(vis, pool_id, listed, occupancy)
    exp, exp_counts = lsup.select_expected(twin, fetched, scales, ids, sizes, lod)
    vis.select_lods(pool_id, scales)
    got, counts = vis.lods(pool_id)  # waits for the selection
    assert counts.shape == (len(listed), GV_MAX_LOD_LEVELS) and counts.tolist() == exp_counts.tolist()
    for v, f in enumerate(fetched):
        assert int(counts[v].sum()) == int(f["draw_count"])
        assert got[v].tolist() == exp[v].tolist(), v
    return fetched, exp, exp_counts


def commands(vis, fetched, draw_ids, table, dtype, merge=False, region=0, draws=False, own=True, pool_id=0):
    """Emits the commands of the pool's last instance emission behind its selection and compares every byte on the device and of a
    host fetch, and the counts, with the restatement given the per-DRAW ids. Returns (expected bytes, counts)."""
    import torch
    starts = instance_starts(vis, pool_id)
    bases = vis.draw_bases(pool_id) if draws else None
    stride = dtype.itemsize
    rows = (len(fetched) * region if region else sum(int(f["draw_count"]) for f in fetched)) + 7
    pattern = csup.background(rows, stride)
    exp, counts = lsup.expected_commands(fetched, starts, bases, draw_ids, table, dtype, merge, region, None, pattern)
    vis.set_command_layout(pool_id, dtype=dtype)
    if own:
        dev = torch.full((rows, stride), csup.BACKGROUND, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()  # (torch's stream; the library's stream is non-blocking)
        vis.emit_draw_commands(pool_id, merge, region, device=(dev.data_ptr(), rows * stride))
    else:
        vis.emit_draw_commands(pool_id, merge, region)
    host = pattern.copy()
    _, got_counts = vis.draw_commands(pool_id, out=host)  # waits for the emission
    assert got_counts.tolist() == counts.tolist()
    assert host.tobytes() == exp.tobytes()
    if own:
        assert dev.cpu().numpy().tobytes() == exp.tobytes()
    return exp, counts


def id_mirror_commands(vis, fetched, ids, table, dtype, merge=False, pool_id=0):
    """the command emission WITHOUT a selection: the per-slot ids (commands_support.expected)"""
    starts = instance_starts(vis, pool_id)
    rows = sum(int(f["draw_count"]) for f in fetched) + 7
    pattern = csup.background(rows, dtype.itemsize)
    exp, counts = csup.expected(fetched, starts, None, ids, table, dtype, merge, 0, None, pattern)
    vis.set_command_layout(pool_id, dtype=dtype)
    vis.emit_draw_commands(pool_id, merge)
    host = pattern.copy()
    _, got_counts = vis.draw_commands(pool_id, out=host)
    assert got_counts.tolist() == counts.tolist() and host.tobytes() == exp.tobytes()
    return exp


# ---- 1. workgroup and chunk edges, both emission forms, both command modes ---------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_selection_and_commands_at_workgroup_and_chunk_edges(n, twin):
    """4 levels, 7 base geometries (28 table entries at stride 4); emit_instances -> select -> commands in both modes, then
    emit_draw_instances with ready counts 0 .. 5 -> select -> commands in both modes"""
    w = World(n)
    rng = np.random.Generator(np.random.PCG64(n))
    ready = np.ones(n, np.uint32)
    with GpuVisibility(device=0) as vis:
        bind(vis, w.scene)
        vis.bind_ready(0, ready)
        vis.bind_geometry(0, w.ids, w.table)
        vis.bind_lod(0, w.sizes, w.lod)
        vis.cull(0, [enclosing()])
        whole_world(fetch_all(vis, 0, [0], n)[0], n)
        vis.set_instance_layout(0, dtype=isup.BARE)
        vis.emit_instances(0, [0])
        fetched, g, counts = select(vis, twin, [0], n, [1.0], w.ids, w.sizes, w.lod)
        balanced(counts[0], n, w.levels)
        assert ((g[0] - w.ids[fetched[0]["visible_idx"]]) < w.levels).all()
        commands(vis, fetched, g, w.table, csup.INDEXED)
        commands(vis, fetched, g, w.table, csup.GAPS, merge=True)
        commands(vis, fetched, g, w.table, csup.INDEXED, own=False)
        ready[:] = rng.integers(0, 6, n, dtype=np.uint32)
        vis.mark_dirty(GV_DIRTY_MESH, 0, n, pool_id=0)
        vis.emit_draw_instances(0, [0])
        assert code(vis.lods_device, 0) == GV_E_STATE  # the selection belonged to the emission in front of it
        fetched, g, counts = select(vis, twin, [0], n, [1.0], w.ids, w.sizes, w.lod)
        whole_world(fetched[0], n)
        exp, _ = commands(vis, fetched, g, w.table, csup.INDEXED, draws=True)
        got = exp[:n].reshape(-1).view(csup.INDEXED)
        assert got["instance_count"].tolist() == ready[fetched[0]["visible_idx"]].tolist()
        commands(vis, fetched, g, w.table, csup.GAPS, merge=True, draws=True)


# ---- 2. eight views, eight scales -----------------------------------------------------------------------------------------------

def test_eight_views_eight_scales_and_shared_cameras_agree(twin):
    n = 3000
    w = World(n)
    side = 100.0 * n ** (1.0 / 3.0)
    part = lambda k, **kw: scene.make_view(scene.ortho_rev_z(0.7 * side, 0.7 * side, -side, side), shadow_pass=k, **kw)
    nothing = scene.make_view(scene.ortho_rev_z(10.0, 10.0, -5.0, 5.0), camera_position=(50.0 * side, 0.0, 0.0), shadow_pass=2)
    views = [enclosing(),                                      # the main pass
             enclosing(shadow_pass=0, camera_offset=(3.5, -2.0, 1.25)),  # a cascade that shares its camera_position
             part(1), nothing,
             enclosing(shadow_pass=3), part(4),
             enclosing(shadow_pass=5, camera_position=(250.0, -100.0, 50.0)),  # another camera: other distances
             part(6, camera_position=(-40.0, 10.0, 5.0))]
    subnormal = np.float32(1e-40)
    scales = np.array([1.0, 1.0, 0.0, 0.25, np.inf, np.nan, subnormal, 4.0], np.float32)
    assert subnormal > 0 and subnormal < np.finfo(np.float32).tiny
    listed = list(range(8))
    with GpuVisibility(device=0) as vis:
        bind(vis, w.scene)
        vis.bind_geometry(0, w.ids, w.table)
        vis.bind_lod(0, w.sizes, w.lod)
        vis.cull(0, views)
        vis.set_instance_layout(0, dtype=isup.BARE)
        vis.emit_instances(0, listed)
        fetched, g, counts = select(vis, twin, listed, n, scales, w.ids, w.sizes, w.lod)
        whole_world(fetched[0], n)
        seen = [int(f["draw_count"]) for f in fetched]
        assert seen[0] == seen[1] == seen[4] == seen[6] == n and seen[3] == 0 and 100 < seen[2] < n - 100 and 100 < seen[5] < n - 100
        balanced(counts[0], n, w.levels)
        # a main view and a cascade that share camera_position and scale agree slot by slot
        by_slot = lambda v: g[v][np.argsort(fetched[v]["visible_idx"][:seen[v]], kind="stable")]
        assert by_slot(0).tolist() == by_slot(1).tolist()
        assert by_slot(0).tolist() != by_slot(6).tolist()  # (another camera, another scale: other levels)
        # scale 0: x = 0 exceeds nothing; inf: everything; NaN: nothing
        assert counts[2].tolist() == [seen[2]] + [0] * 7 and counts[5].tolist() == [seen[5]] + [0] * 7
        assert counts[4].tolist() == [0, 0, 0, n, 0, 0, 0, 0]
        assert counts[3].tolist() == [0] * 8 and counts[6].tolist() == [n] + [0] * 7  # (a subnormal scale: x below every q)
        commands(vis, fetched, g, w.table, csup.GAPS)
        commands(vis, fetched, g, w.table, csup.GAPS, merge=True)
        commands(vis, fetched, g, w.table, csup.INDEXED, merge=True, region=n + 10, own=False)


# ---- 3. a sorted view ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("descending", [False, True])
def test_levels_follow_the_sorted_models_and_runs_are_few(descending, twin):
    """one geometry of 4 levels and one size: behind a sort by distance the levels are monotone, so run mode writes a handful of
    commands"""
    n = 5000
    w = World(n, bases=1)
    sizes = np.full(n, 2.0, np.float32)
    lod = lsup.lod_table([(4, lsup.quantile_thresholds(w.scene.transforms["position"], sizes, 4))] + [(1, [])] * 3)
    ids = np.zeros(n, np.uint32)
    with GpuVisibility(device=0) as vis:
        bind(vis, w.scene)
        vis.bind_geometry(0, ids, w.table)
        vis.bind_lod(0, sizes, lod)
        vis.cull(0, [enclosing()])
        unsorted = fetch_all(vis, 0, [0], n)[0]["visible_idx"].copy()
        vis.sort(0, descending=descending, pool_id=0)
        vis.set_instance_layout(0, dtype=isup.BARE)
        vis.emit_instances(0, [0])
        fetched, g, counts = select(vis, twin, [0], n, [1.0], ids, sizes, lod)
        whole_world(fetched[0], n)
        steps = np.diff(fetched[0]["distance_sq"])
        assert ((steps <= 0) if descending else (steps >= 0)).all() and fetched[0]["visible_idx"].tolist() != unsorted.tolist()
        balanced(counts[0], n, 4)
        runs = 1 + int(np.count_nonzero(np.diff(g[0].astype(np.int64))))  # the CPU restatement first
        assert runs < n / 4
        level_steps = np.diff(g[0].astype(np.int64))
        assert ((level_steps <= 0) if descending else (level_steps >= 0)).all()
        _, command_counts = commands(vis, fetched, g, w.table, csup.GAPS, merge=True)
        assert int(command_counts[0]) == runs and int(command_counts[0]) < n / 4
        commands(vis, fetched, g, w.table, csup.INDEXED)


# ---- 4. planted extremes ---------------------------------------------------------------------------------------------------------

def test_planted_extremes(twin):
    """sizes that are NaN, +-inf, subnormal, -1 and 0; pivots whose d2 overflows; exact ties and their one-ulp neighbours at lanes
    0, 63, 64, 255 / 1, 62, 65, 254; levels 1 and 8; base ids at and beyond lod_table_count; base ids whose b + level leaves the
    geometry table. Under 25 % of the world is planted."""
    n = 2048
    half = 1.0e21  # (the view also holds the far pivots)
    w = World(n, bases=3)  # geometry 0, 4, 8 with 4 levels
    rng = np.random.Generator(np.random.PCG64(4))
    planted = rng.permutation(n)[:400]
    position = w.scene.transforms["position"]
    ids, sizes = w.ids.copy(), w.sizes.copy()
    for k, value in enumerate([np.nan, np.inf, -np.inf, 1e-40, -1.0, 0.0]):
        sizes[planted[10 * k:10 * k + 10]] = np.float32(value)
    far = planted[60:70]
    position[far, 0], position[far, 2] = 3.0e19, -3.0e19  # d2 = 1.8e39: +inf in fp32
    eighths = lsup.quantile_thresholds(position, w.sizes, 8)
    rows = [(4, w.switch_at) if g % 4 == 0 else (1, []) for g in range(12)]
    rows += [(1, []),                                   # 12: one level
             (2, [5.0]),                                # 13: the tie
             (8, eighths),                              # 14: eight levels
             (2, [np.nextafter(np.float32(5.0), np.float32(0.0))]),  # 15: one ulp below the tie
             (8, [1e-6 * (j + 1) for j in range(7)])]   # 16: eight levels, all switched: 16 + 7 leaves the geometry table
    lod = lsup.lod_table(rows)
    table = random_table(20)
    ids[planted[70:100]] = 12
    ids[planted[100:200]] = 14
    ids[planted[200:230]] = 16
    ids[planted[230:240]] = len(lod)            # at lod_table_count: one level, geometry 17
    ids[planted[240:250]] = len(lod) + 1
    ids[planted[250:260]] = 70000               # beyond both tables
    ids[planted[260:270]] = 0xFFFFFFFF
    with GpuVisibility(device=0) as vis:
        bind(vis, w.scene)
        vis.bind_geometry(0, ids, table)
        vis.bind_lod(0, sizes, lod)
        vis.cull(0, [enclosing(half)])
        order = fetch_all(vis, 0, [0], n)[0]
        whole_world(order, n)
        # the ties go where the lanes are: the mirror keeps its order under a transform edit
        ties, ulps = order["visible_idx"][[0, 63, 64, 255]], order["visible_idx"][[1, 62, 65, 254]]
        for slots, base in ((ties, 13), (ulps, 15)):
            position[slots, :3] = (3.0, 4.0, 0.0)
            sizes[slots], ids[slots] = 1.0, base
        for slot in np.concatenate([ties, ulps]):
            vis.mark_dirty(GV_DIRTY_TRANSFORM, int(slot), 1)
        vis.cull(0, [enclosing(half)])
        vis.set_instance_layout(0, dtype=isup.BARE)
        vis.emit_instances(0, [0])
        fetched, g, counts = select(vis, twin, [0], n, [1.0], ids, sizes, lod)
        whole_world(fetched[0], n)
        slots = fetched[0]["visible_idx"]
        assert slots.tolist() == order["visible_idx"].tolist()
        assert fetched[0]["baked_model"].reshape(-1, 12)[[0, 63, 64, 255, 1, 62, 65, 254], 9:12].tolist() == [[3.0, 4.0, 0.0]] * 8
        of = dict(zip(slots.tolist(), g[0].tolist()))
        assert [of[int(s)] for s in ties] == [13] * 4 and [of[int(s)] for s in ulps] == [16] * 4
        special = set(ties.tolist()) | set(ulps.tolist())
        rest = lambda group: [int(s) for s in group if int(s) not in special]
        assert all(of[s] == int(ids[s]) for s in rest(planted[0:10]))               # NaN size: the finest
        assert all(of[s] == int(ids[s]) + 3 for s in rest(far))                     # d2 = +inf: the coarsest (4 levels, finite sizes)
        assert all(of[s] == 12 for s in rest(planted[70:100]))                      # one level
        assert len({of[s] for s in rest(planted[100:200])}) >= 6                    # eight levels in use
        assert all(of[s] == 23 for s in rest(planted[200:230]))                     # leaves the geometry table
        assert all(of[s] == int(ids[s]) for s in rest(planted[230:270]))            # ids outside the LOD table: level 0
        assert len(planted) < n / 4
        for merge in (False, True):
            exp, command_counts = commands(vis, fetched, g, table, csup.GAPS, merge)
            got = exp[:int(command_counts[0])].reshape(-1).view(csup.GAPS)
            void = got[np.isin(got["draw"], np.nonzero(g[0] >= len(table))[0])]
            assert len(void) >= (40 if not merge else 1) and not void["count"].any() and not void["instance_count"].any()


# ---- 5. currency -----------------------------------------------------------------------------------------------------------------

def test_marks_are_consumed_by_the_selection_and_not_by_the_commands_behind_it(twin):
    n = 3000
    w = World(n)
    ids, sizes = w.ids, w.sizes
    with GpuVisibility(device=0) as vis:
        bind(vis, w.scene)
        vis.bind_geometry(0, ids, w.table)
        vis.bind_lod(0, sizes, w.lod)
        vis.cull(0, [enclosing()])
        vis.set_instance_layout(0, dtype=isup.BARE)
        vis.emit_instances(0, [0])
        uploaded = lambda: vis.stats()["upload_bytes"]
        before = uploaded()
        fetched, g0, counts = select(vis, twin, [0], n, [1.0], ids, sizes, w.lod)
        whole_world(fetched[0], n)
        balanced(counts[0], n, w.levels)
        assert uploaded() - before == 2 * n * 4  # the first selection uploads both columns
        # sizes changed after the cull, marked GV_DIRTY_LOD, then GV_DIRTY_MESH: three single slots travel as one packet [sizes | slots]
        # (a mesh mark also feeds the id mirror's dirty set: a second packet); a huge size is the finest level, a tiny one the coarsest
        level_of = lambda g, slot: int(g[0][fetched[0]["visible_idx"].tolist().index(slot)]) - int(ids[slot])
        for kind, value, level, packets in ((GV_DIRTY_LOD, 1.0e6, 0, 1), (GV_DIRTY_MESH, 1.0e-6, w.levels - 1, 2)):
            before = uploaded()
            for slot in (5, 900, 2000):
                sizes[slot] = np.float32(value)
                vis.mark_dirty(kind, slot, 1, pool_id=0)
            _, g1, _ = select(vis, twin, [0], n, [1.0], ids, sizes, w.lod)
            assert uploaded() - before == packets * 3 * 8
            assert [level_of(g1, slot) for slot in (5, 900, 2000)] == [level] * 3
            assert g1[0].tolist() != g0[0].tolist()
            g0 = g1
        # an id changed under GV_DIRTY_GEOMETRY
        before = uploaded()
        ids[[7, 1500]] = (ids[[7, 1500]] + 4) % 28
        vis.mark_dirty(GV_DIRTY_GEOMETRY, 7, 1, pool_id=0)
        vis.mark_dirty(GV_DIRTY_GEOMETRY, 1500, 1, pool_id=0)
        _, g1, _ = select(vis, twin, [0], n, [1.0], ids, sizes, w.lod)
        assert uploaded() - before == 2 * 8 and g1[0].tolist() != g0[0].tolist()
        commands(vis, fetched, g1, w.table, csup.INDEXED)
        # marks made AFTER the selection are not seen by the command emission that follows ...
        ids[[9, 1700]] = (ids[[9, 1700]] + 8) % 28
        sizes[11] *= np.float32(1024.0)
        vis.mark_dirty(GV_DIRTY_GEOMETRY, 9, 1, pool_id=0)
        vis.mark_dirty(GV_DIRTY_GEOMETRY, 1700, 1, pool_id=0)
        vis.mark_dirty(GV_DIRTY_LOD, 11, 1, pool_id=0)
        commands(vis, fetched, g1, w.table, csup.INDEXED)
        commands(vis, fetched, g1, w.table, csup.GAPS, merge=True)
        # ... the next selection sees them
        _, g2, _ = select(vis, twin, [0], n, [1.0], ids, sizes, w.lod)
        assert g2[0].tolist() != g1[0].tolist()
        commands(vis, fetched, g2, w.table, csup.INDEXED)
        # gv_sync consumes the marks too
        sizes[13] *= np.float32(1024.0)
        vis.mark_dirty(GV_DIRTY_LOD, 13, 1, pool_id=0)
        before = uploaded()
        vis.sync()
        assert uploaded() - before >= 8
        vis.cull(0, [enclosing()])
        vis.emit_instances(0, [0])
        before = uploaded()
        select(vis, twin, [0], n, [1.0], ids, sizes, w.lod)
        assert uploaded() == before
        # a rebind re-uploads: the table at the bind, the column at the next selection
        other = (sizes * np.float32(0.5)).astype(np.float32)
        before = uploaded()
        vis.bind_lod(0, other, w.lod)
        assert uploaded() - before == len(w.lod) * 32
        _, g3, _ = select(vis, twin, [0], n, [1.0], ids, other, w.lod)
        assert uploaded() - before == len(w.lod) * 32 + n * 4
        # sizes == NULL selects by distance alone, and no mirror is kept
        before = uploaded()
        vis.bind_lod(0, None, w.lod)
        _, g4, _ = select(vis, twin, [0], n, [1.0], ids, None, w.lod)
        assert uploaded() - before == len(w.lod) * 32 and g4[0].tolist() != g3[0].tolist()
        commands(vis, fetched, g4, w.table, csup.INDEXED, merge=True)


# ---- 6. nothing else moves -------------------------------------------------------------------------------------------------------

def test_results_and_instances_stay_launches_are_counted_and_the_selection_ends_with_its_emission(twin):
    n = 5000
    w = World(n)
    views = [enclosing(), scene.cascade_view(index=0, size=400.0)]
    with GpuVisibility(device=0) as vis:
        bind(vis, w.scene)
        vis.bind_geometry(0, w.ids, w.table)
        vis.bind_lod(0, w.sizes, w.lod)
        vis.cull(0, views)
        vis.set_instance_layout(0, dtype=isup.FULL)
        vis.emit_instances(0, [0, 1])
        vis.set_command_layout(0, dtype=csup.INDEXED)
        results, (instances, starts) = fetch_all(vis, 0, [0, 1], n), vis.instances(0)
        whole_world(results[0], n)
        plain = id_mirror_commands(vis, results, w.ids, w.table, csup.INDEXED)  # (uploads the ids: not counted as launches)
        fetched, g, _ = select(vis, twin, [0, 1], n, [1.0, 0.5], w.ids, w.sizes, w.lod)  # (uploads the sizes)
        for _ in range(2):
            before = launches(vis)
            vis.select_lods(0, [1.0, 0.5])
            assert launches(vis) - before == 1
        for merge, grown in ((False, 1), (True, 3)):
            before = launches(vis)
            vis.emit_draw_commands(0, merge_runs=merge)
            assert launches(vis) - before == grown
            vis.draw_commands(0)
        for a, b in zip(results, fetch_all(vis, 0, [0, 1], n)):
            isup.same_results(a, b)
        again, again_starts = vis.instances(0)
        assert again.tobytes() == instances.tobytes() and again_starts.tolist() == starts.tolist()
        selected, _ = commands(vis, fetched, g, w.table, csup.INDEXED, own=False)
        assert selected.tobytes() != plain.tobytes()
        # dropping the selection gives back the id-mirror commands byte for byte
        vis.select_lods(0, None)
        assert code(vis.lods_device, 0) == GV_E_STATE
        assert id_mirror_commands(vis, results, w.ids, w.table, csup.INDEXED).tobytes() == plain.tobytes()
        # an instance emission drops it too
        select(vis, twin, [0, 1], n, [1.0, 0.5], w.ids, w.sizes, w.lod)
        assert vis.lods_device(0)[0]
        vis.emit_instances(0, [0, 1])
        assert code(vis.lods_device, 0) == GV_E_STATE
        assert id_mirror_commands(vis, results, w.ids, w.table, csup.INDEXED).tobytes() == plain.tobytes()
        # ... and so does gv_cull
        select(vis, twin, [0, 1], n, [1.0, 0.5], w.ids, w.sizes, w.lod)
        vis.cull(0, views)
        assert code(vis.lods_device, 0) == GV_E_STATE and code(vis.lods, 0) == GV_E_STATE


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------

def test_error_codes_each_followed_by_a_correct_selection(twin):
    n = 1200
    w = World(n)
    views = [enclosing(), scene.cascade_view(index=0, size=400.0)]
    with GpuVisibility(device=0) as vis:
        bind(vis, w.scene)
        vis.cull(0, views)
        vis.set_instance_layout(0, dtype=isup.BARE)
        lib, ctx = vis.lib, vis.ctx

        def good():
            vis.bind_geometry(0, w.ids, w.table)
            vis.bind_lod(0, w.sizes, w.lod)
            vis.emit_instances(0, [0, 1])
            fetched, g, _ = select(vis, twin, [0, 1], n, [1.0, 2.0], w.ids, w.sizes, w.lod)
            commands(vis, fetched, g, w.table, csup.INDEXED, merge=True)

        # gv_pool_bind_lod
        rows = (GvLodGeometry * 3)()
        for r in rows:
            r.levels = 2
        none_levels, nine_levels = (GvLodGeometry * 3)(), (GvLodGeometry * 3)()
        for a, b in zip(none_levels, nine_levels):
            a.levels, b.levels = 1, 1
        none_levels[1].levels, nine_levels[2].levels = 0, 9
        sizes = w.sizes.ctypes.data
        for args in ((99, sizes, 4, n, rows, 3),                          # a pool out of range
                     (0, sizes, 2, n, rows, 3),                           # stride < 4
                     (0, sizes, 4, n, None, 0),                           # sizes without a table
                     (0, sizes, 4, n, None, 3),                           # a NULL table with table_count > 0
                     (0, sizes, 4, n, rows, 0),                           # table_count 0 with a table
                     (0, None, 0, 0, rows, GV_MAX_GEOMETRIES + 1),        # table_count above the limit
                     (0, sizes, 4, n, none_levels, 3),                    # levels 0
                     (0, sizes, 4, n, nine_levels, 3),                    # levels 9
                     (0, sizes, 4, 1 << 28, rows, 3)):                    # an occupancy beyond the 28-bit slot range
            assert lib.gv_pool_bind_lod(ctx, *args) == GV_E_ARG, args
        good()
        # gv_pool_select_lods: GV_E_ARG
        assert code(vis.select_lods, 99, [1.0, 1.0]) == GV_E_ARG                             # a pool out of range
        assert lib.gv_pool_select_lods(ctx, 0, None, 2) == GV_E_ARG                          # no scales for two views
        assert code(vis.select_lods, 0, [1.0]) == GV_E_ARG                                   # view_count other than the emission's
        assert code(vis.select_lods, 0, [1.0, 1.0, 1.0]) == GV_E_ARG
        good()
        # ... GV_E_STATE
        vis.bind_lod(0, None, None)
        assert code(vis.select_lods, 0, [1.0, 1.0]) == GV_E_STATE                            # no LOD binding
        vis.bind_lod(0, w.sizes, w.lod)
        vis.bind_geometry(0, None, None)
        assert code(vis.select_lods, 0, [1.0, 1.0]) == GV_E_STATE                            # no geometry binding
        vis.bind_geometry(0, w.ids[:n - 1], w.table)
        assert code(vis.select_lods, 0, [1.0, 1.0]) == GV_E_STATE                            # an id column below a view's occupancy
        vis.bind_geometry(0, w.ids, w.table)
        vis.bind_lod(0, w.sizes[:n - 1], w.lod)
        assert code(vis.select_lods, 0, [1.0, 1.0]) == GV_E_STATE                            # a size column below a view's occupancy
        vis.bind_lod(0, w.sizes, w.lod)
        vis.cull(0, views)
        assert code(vis.select_lods, 0, [1.0, 1.0]) == GV_E_STATE                            # no emission since the last gv_cull
        assert code(vis.lods_device, 0) == GV_E_STATE
        good()
        # flags == 2 stays an error behind a selection
        assert code(vis.emit_draw_commands, 0, flags=2) == GV_E_ARG
        # the fetch: too small an array writes nothing
        small, counts = np.full(40, 0xA5A5A5A5, np.uint32), np.full(16, 0xA5A5A5A5, np.uint32)
        assert lib.gv_pool_lods_fetch(ctx, 0, small.ctypes.data_as(U32P), len(small), counts.ctypes.data_as(U32P), 16) == GV_E_ARG
        assert lib.gv_pool_lods_fetch(ctx, 0, None, 0, counts.ctypes.data_as(U32P), 15) == GV_E_ARG
        assert (small == 0xA5A5A5A5).all() and (counts == 0xA5A5A5A5).all()
        good()


# ---- 8. the drop-in's shim -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lod_commands_driver(tmp_path_factory):
    """tests/cpp/lod_commands.cpp, built with the flags of the headless_tick rule of tests/cpp/Makefile"""
    cpp, lib = os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "garden_amd", "lib")
    exe = str(tmp_path_factory.mktemp("lod_commands") / "lod_commands")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-invalid-offsetof", "-fno-strict-aliasing", "-march=haswell",
                    "-ffp-contract=off", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(cpp, "lod_commands.cpp"),
                    "-o", exe, "-L" + lib, "-lgarden_vis", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64",
                    "-lm", "-lpthread"], check=True)
    return exe


def test_lod_shim_matches_the_host_loop(lod_commands_driver):
    """GpuInstanceWriter + GpuDrawCommands with setLods / setLodScale against a host loop over the records in draw order that picks
    each draw's level with the twin: 30 000 entities in three mesh systems (one without levels, one with 4, one sorted with 8), main
    pass + three cascades, 20 ticks with movers, geometry switches and size edits — every command array byte for byte, in both
    modes; every one of the eight levels is drawn."""
    p = subprocess.run([lod_commands_driver, "--entities", "30000", "--ticks", "20"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["ok"] and out["systems"] == 3 and out["passes"] == 4 and out["ticks"] == 20 and out["commands"] > 100_000, out
    assert all(count > 0 for count in out["levels"]), out
