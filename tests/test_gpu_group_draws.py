"""gv_pool_group_draws on the device: a view's records reordered by geometry key, stable. Expected values are exact: the records are
fetched in front of the call, kappa is computed on the host (with GV_GROUP_BY_LOD through the C twin of the LOD rule,
tests/lod_twin.h), np.argsort(kappa, kind="stable") gives the order, and all three fetched arrays are compared afterwards, the floats
as bit patterns. Every case first asserts, on that CPU restatement, the conditions that keep it from passing by accident
(tests/group_support.check_conditions). Where a deferred sort must still be pending when the call is issued, the records in front of
the call come from a second context that ran the same frame up to there.

The world is the flat pool of tests/test_gpu_lod_select.py under an enclosing view, so draw_count == N."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import commands_support as csup
import delivery_support as dsup
import group_support as gsup
import instances_support as isup
import lod_support as lsup
from garden_amd import scene
from garden_amd.lib import (GV_DIRTY_GEOMETRY, GV_DIRTY_LOD, GV_E_ARG, GV_E_STATE, GV_GROUP_BY_LOD, GpuVisibility, GvError)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32P = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return lsup.build_twin(tmp_path_factory.mktemp("lod_twin"))


def enclosing(half=1.0e7, shadow_pass=-1):
    """an orthographic view that holds the whole scene: every box becomes a draw"""
    return scene.make_view(scene.ortho_rev_z(2 * half, 2 * half, -half, half), shadow_pass=shadow_pass)


def nothing_view(shadow_pass=-1):
    return scene.make_view(scene.ortho_rev_z(10.0, 10.0, -5.0, 5.0), camera_position=(1.0e9, 0.0, 0.0), shadow_pass=shadow_pass)


def bind(vis, sc, pool_id=0):
    vis.bind_transforms(sc.transforms, sc.entity_to_transform)
    vis.bind_pool(pool_id, sc.meshes)
    vis.hierarchy_rebuild()


def fetch(vis, n, view=0, pool_id=0):
    return vis.fetch(view, write_back=False, occupancy=n, order="raw", pool_id=pool_id)


def sort_launches(vis):
    return vis.stats()["launches"]["sort"]


def code(fn, *args, **kw):
    with pytest.raises(GvError) as e:
        fn(*args, **kw)
    return e.value.code


class Setup:
    """a case's world: scene, ids, geometry table, and the LOD world where the case groups by level"""

    def __init__(self, c):
        self.c = c
        self.scene = scene.flat_scene(c.n, defects=False)
        self.lodw = gsup.LodWorld(self.scene.transforms["position"]) if c.by_lod else None
        self.ids = (self.lodw.ids if c.width else None) if c.by_lod else gsup.case_ids(c)
        self.table = self.lodw.table if c.by_lod else gsup.geometry_table(c.K)
        assert len(self.table) == c.K

    def open(self, vis):
        bind(vis, self.scene)
        vis.bind_geometry(0, self.ids, self.table)
        if self.lodw:
            vis.bind_lod(0, self.lodw.sizes, self.lodw.lod)
        vis.cull(0, [enclosing()])
        if self.c.presort:
            vis.sort(0, pool_id=0)

    def kappa(self, before, twin, scale=1.0):
        lod = (twin, before["baked_model"], self.lodw.sizes, scale, self.lodw.lod) if self.lodw else None
        return gsup.keys(before["visible_idx"], self.ids, self.c.K, lod)


# ---- 1. every count, key width, id width and LOD key of the case table ---------------------------------------------------------------

@pytest.mark.parametrize("case", gsup.CASES, ids=lambda c: c.name)
def test_grouped_records_equal_the_stable_argsort_of_the_keys(case, twin):
    c, s = case, Setup(case)
    with GpuVisibility(device=0) as vis:
        s.open(vis)
        if c.presort:  # the records in front of the call from a context of its own: here the deferred sort stays pending
            with GpuVisibility(device=0) as other:
                s.open(other)
                before = fetch(other, c.n)
        else:
            before = fetch(vis, c.n)
        assert int(before["draw_count"]) == c.n
        kappa = s.kappa(before, twin)
        gsup.check_conditions(kappa, None if c.presort else before["visible_idx"])
        order = gsup.order_of(kappa)
        exp = gsup.expected_results(before, order)
        launched = sort_launches(vis)
        vis.group_draws(0, pool_id=0, by_lod=c.by_lod, view_scale=1.0)
        if not c.presort:
            assert sort_launches(vis) - launched == 2 * gsup.digits(c.K)  # fixed by the host from K
        after = fetch(vis, c.n)
        gsup.same_records(after, exp, c.n)
        assert int(after["instance_count"]) == int(before["instance_count"])
        if c.presort:  # behind the sort every group is still in distance order
            grouped = kappa[order].astype(np.int64)
            steps = np.diff(after["distance_sq"])
            assert (steps[np.diff(grouped) == 0] >= 0).all()
            assert (np.diff(before["distance_sq"]) >= 0).all() and (steps < 0).any()
        # grouping twice is grouping once
        vis.group_draws(0, pool_id=0, by_lod=c.by_lod, view_scale=1.0)
        gsup.same_records(fetch(vis, c.n), exp, c.n)


def test_a_view_that_sees_nothing_and_its_sibling(twin):
    """two views of one pool: the grouped one sees nothing (device count 0), then the other one is grouped while the first, ungrouped
    now, stays bit-identical; a grouped view is refused by gv_merge_sorted"""
    c = gsup.CASE_BY_NAME["count-2049"]
    s = Setup(c)
    dt = dsup.LAYOUTS["packed_sorted"][0]
    with GpuVisibility(device=0) as vis:
        bind(vis, s.scene)
        vis.bind_geometry(0, s.ids, s.table)
        vis.cull(0, [enclosing(), nothing_view(0), enclosing(shadow_pass=1)])
        vis.group_draws(1, pool_id=0)
        empty = fetch(vis, c.n, view=1)
        assert int(empty["draw_count"]) == 0
        before = [fetch(vis, c.n, view=v) for v in (0, 2)]
        kappa = gsup.keys(before[0]["visible_idx"], s.ids, c.K)
        gsup.check_conditions(kappa, before[0]["visible_idx"])
        vis.sort(0, pool_id=0)
        vis.sort(2, pool_id=0)
        sorted_before = [fetch(vis, c.n, view=v) for v in (0, 2)]
        vis.group_draws(0, pool_id=0)
        kappa = gsup.keys(sorted_before[0]["visible_idx"], s.ids, c.K)
        gsup.same_records(fetch(vis, c.n, view=0), gsup.expected_results(sorted_before[0], gsup.order_of(kappa)), c.n)
        isup.same_results(fetch(vis, c.n, view=2), sorted_before[1])  # the ungrouped view: bit-identical
        group = lambda views: [dict(group_id=0, items=[(0, v, v, 1) for v in views], descending=False, dtype=dt)]
        assert code(vis.merge_sorted, group([0, 2])) == GV_E_STATE  # view 0 no longer counts as sorted
        vis.merge_sorted(group([2]))                                # ... view 2 still does
        vis.sort(0, pool_id=0)                                      # a later sort orders it by distance again
        vis.merge_sorted(group([0, 2]))
        isup.same_results(fetch(vis, c.n, view=0), sorted_before[0])  # group then sort equals sort alone


def test_no_id_column_without_the_flag_launches_nothing():
    n = 3000
    sc = scene.flat_scene(n, defects=False)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_geometry(0, None, gsup.geometry_table(5))
        vis.cull(0, [enclosing()])
        before = fetch(vis, n)
        launched = sum(vis.stats()["launches"].values())
        vis.group_draws(0, pool_id=0, view_scale=float("nan"))  # (ignored without the flag)
        assert sum(vis.stats()["launches"].values()) == launched
        isup.same_results(fetch(vis, n), before)


# ---- 2. a later selection selects the grouped keys -----------------------------------------------------------------------------------

def planted_lod_world(n):
    sc = scene.flat_scene(n, defects=False)
    w = gsup.LodWorld(sc.transforms["position"])
    rng = np.random.Generator(np.random.PCG64(n))
    at = rng.permutation(n)
    w.sizes[at[:5]] = np.float32(np.nan)            # a NaN size: the finest level
    sc.transforms["position"][at[5:10], 0] = 3.0e19  # d2 = +inf in fp32: the coarsest
    sc.transforms["position"][at[5:10], 2] = -3.0e19
    return sc, w, at


@pytest.mark.parametrize("scale", [1.0, 0.25])
def test_a_later_selection_returns_the_grouped_keys(scale, twin):
    """4 levels, 7 bases, a NaN size and an infinite distance planted: gv_pool_select_lods behind a later emission, with the same
    scale, returns ids equal to the grouped keys, non-decreasing over the view; run mode writes one command per id + level"""
    n = 5000
    sc, w, at = planted_lod_world(n)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_geometry(0, w.ids, w.table)
        vis.bind_lod(0, w.sizes, w.lod)
        vis.cull(0, [enclosing(1.0e21)])
        before = fetch(vis, n)
        assert int(before["draw_count"]) == n
        kappa = gsup.keys(before["visible_idx"], w.ids, len(w.table), (twin, before["baked_model"], w.sizes, scale, w.lod))
        gsup.check_conditions(kappa, before["visible_idx"])
        of = dict(zip(before["visible_idx"].tolist(), kappa.tolist()))
        assert all(of[int(s)] == int(w.ids[s]) for s in at[:5]) and all(of[int(s)] == int(w.ids[s]) + 3 for s in at[5:10])
        order = gsup.order_of(kappa)
        vis.group_draws(0, pool_id=0, by_lod=True, view_scale=scale)
        after = fetch(vis, n)
        gsup.same_records(after, gsup.expected_results(before, order), n)
        vis.set_instance_layout(0, dtype=isup.FULL)
        vis.emit_instances(0, [0])
        vis.select_lods(0, [scale])
        g, counts = vis.lods(0)
        assert g[0].tolist() == kappa[order].tolist() and (np.diff(g[0].astype(np.int64)) >= 0).all()
        assert int(counts[0].sum()) == n
        distinct = len(np.unique(kappa))
        commands_equal_the_restatement(vis, [after], [g[0]], w.table, n, distinct, per_draw=True)
        instances, _ = vis.instances(0, dtype=isup.FULL)
        assert instances["slot"].tolist() == after["visible_idx"].tolist()


def commands_equal_the_restatement(vis, fetched, ids, table, n, distinct, per_draw=False, draws=False, pool_id=0):
    """run mode behind a grouped view: command_counts == the distinct ids, every byte the restatement's over the fetched grouped
    records, the instance counts sum to the instances of the view"""
    views = vis.instances_info(pool_id)[0]
    starts = np.zeros(views + 1, np.uint32)
    vis._check(vis.lib.gv_pool_instances_fetch(vis.ctx, pool_id, None, 0, starts.ctypes.data_as(U32P), len(starts)))
    bases = vis.draw_bases(pool_id) if draws else None
    pattern = csup.background(n + 7, csup.GAPS.itemsize)
    if per_draw:
        exp, counts = lsup.expected_commands(fetched, starts, bases, ids, table, csup.GAPS, True, 0, None, pattern)
    else:
        exp, counts = csup.expected(fetched, starts, bases, ids, table, csup.GAPS, True, 0, None, pattern)
    vis.set_command_layout(pool_id, dtype=csup.GAPS)
    vis.emit_draw_commands(pool_id, True)
    host = pattern.copy()
    _, got_counts = vis.draw_commands(pool_id, out=host)
    assert got_counts.tolist() == counts.tolist() == [distinct]
    assert host.tobytes() == exp.tobytes()
    got = host[:distinct].reshape(-1).view(csup.GAPS)
    assert int(got["instance_count"].sum()) == int(starts[-1])
    return got


# ---- 3. end to end: group -> instances -> run-mode commands ----------------------------------------------------------------------------

@pytest.mark.parametrize("draws", [False, True])
def test_group_then_emit_then_run_mode_gives_one_command_per_geometry(draws):
    n, K = 6000, 300
    sc = scene.flat_scene(n, defects=False)
    rng = np.random.Generator(np.random.PCG64(n + K))
    ids = rng.integers(0, K, n).astype(np.uint16)  # every id in range
    ready = rng.integers(1, 6, n).astype(np.uint32) if draws else np.ones(n, np.uint32)  # (emit_instances takes one instance per draw)
    table = gsup.geometry_table(K)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_ready(0, ready)
        vis.bind_geometry(0, ids, table)
        vis.cull(0, [enclosing()])
        before = fetch(vis, n)
        kappa = gsup.keys(before["visible_idx"], ids, K)
        gsup.check_conditions(kappa, before["visible_idx"])
        distinct = len(np.unique(kappa))
        # ungrouped, run mode writes about a command per draw
        assert 1 + np.count_nonzero(np.diff(kappa.astype(np.int64))) > n / 2
        vis.group_draws(0, pool_id=0)
        after = fetch(vis, n)
        gsup.same_records(after, gsup.expected_results(before, gsup.order_of(kappa)), n)
        # gv_pool_results_instance_bases follows the new order (ready counts above 1)
        bases = vis.instance_bases(0, 0)
        assert bases.tolist() == np.concatenate([[0], np.cumsum(ready[after["visible_idx"]])]).tolist()
        vis.set_instance_layout(0, dtype=isup.FULL)
        if draws:
            vis.emit_draw_instances(0, [0])
        else:
            vis.emit_instances(0, [0])
        got = commands_equal_the_restatement(vis, [after], ids, table, n, distinct, draws=draws)
        assert (np.diff(got["draw"].astype(np.int64)) > 0).all()
        if draws:
            members = ready[after["visible_idx"]]
            assert got["instance_count"].tolist() == [int(members[kappa[gsup.order_of(kappa)] == k].sum()) for k in np.unique(kappa)]
        else:
            assert got["instance_count"].tolist() == np.unique(kappa, return_counts=True)[1].tolist()
            instances, _ = vis.instances(0, dtype=isup.FULL)
            assert instances["slot"].tolist() == after["visible_idx"].tolist()


# ---- 4. delivery forms -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5000, 300000])
def test_record_structs_and_a_record_target_deliver_the_new_order(n):
    """a record layout (gv_pool_results_records) and a record target, below and above the engine-sized publish"""
    c = gsup.Case("records", n, 4096, 2, 4200, False, False)
    s = Setup(c)
    dt = dsup.LAYOUTS["simd_sorted"][0]
    with GpuVisibility(device=0) as plain:
        s.open(plain)
        before = fetch(plain, n)
    kappa = gsup.keys(before["visible_idx"], s.ids, c.K)
    gsup.check_conditions(kappa, before["visible_idx"])
    exp = gsup.expected_results(before, gsup.order_of(kappa))

    def same(rec, want):
        assert len(rec) == n
        assert rec["componentOffset"].tolist() == (want["visible_idx"].astype(np.uint64) * 48).tolist()
        assert np.ascontiguousarray(rec["bakedModel"]).view(np.uint32).tobytes() == np.ascontiguousarray(want["baked_model"]).view(np.uint32).tobytes()
        assert np.ascontiguousarray(rec["distanceSq"]).view(np.uint32).tobytes() == np.ascontiguousarray(want["distance_sq"]).view(np.uint32).tobytes()
        assert (rec["bufferIndex"] == 5).all()

    for target in (False, True):
        with GpuVisibility(device=0) as vis:
            vis.set_record_layout(0, dt, component_stride=48, buffer_index_value=5)
            mine = np.full(n * dt.itemsize, 0xAB, np.uint8)
            bind(vis, s.scene)
            vis.bind_geometry(0, s.ids, s.table)
            if target:
                vis.set_record_target(0, 0, mine)
            vis.cull(0, [enclosing()])
            fetch(vis, n)
            same(vis.records(0, 0, dt), before)
            vis.group_draws(0, pool_id=0)
            fetch(vis, n)
            same(vis.records(0, 0, dt), exp)
            if target:
                same(mine.view(dt), exp)
                vis.set_record_target(0, 0, None)


# ---- 5. marks, the batch, reproducibility ----------------------------------------------------------------------------------------------

def test_marks_made_between_cull_and_call_are_seen(twin):
    n = 3000
    sc = scene.flat_scene(n, defects=False)
    w = gsup.LodWorld(sc.transforms["position"])
    ids, sizes = w.ids, w.sizes
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_geometry(0, ids, w.table)
        vis.bind_lod(0, sizes, w.lod)
        vis.cull(0, [enclosing()])
        before = fetch(vis, n)
        keys_of = lambda by_lod: gsup.keys(before["visible_idx"], ids, len(w.table), (twin, before["baked_model"], sizes, 1.0, w.lod) if by_lod else None)
        stale = keys_of(False)
        vis.group_draws(0, pool_id=0)  # uploads the id column
        gsup.same_records(fetch(vis, n), gsup.expected_results(before, gsup.order_of(stale)), n)
        # an id edited behind the cull, reported with GV_DIRTY_GEOMETRY
        vis.cull(0, [enclosing()])
        for slot in (7, 1500, 2999):
            ids[slot] = (ids[slot] + 12) % 28
            vis.mark_dirty(GV_DIRTY_GEOMETRY, slot, 1, pool_id=0)
        fresh = keys_of(False)
        assert gsup.order_of(fresh).tolist() != gsup.order_of(stale).tolist()
        uploaded = vis.stats()["upload_bytes"]
        vis.group_draws(0, pool_id=0)
        assert vis.stats()["upload_bytes"] - uploaded == 3 * 8
        gsup.same_records(fetch(vis, n), gsup.expected_results(before, gsup.order_of(fresh)), n)
        # an edited size, reported with GV_DIRTY_LOD
        vis.cull(0, [enclosing()])
        vis.group_draws(0, pool_id=0, by_lod=True)  # uploads the sizes
        stale = keys_of(True)
        gsup.same_records(fetch(vis, n), gsup.expected_results(before, gsup.order_of(stale)), n)
        vis.cull(0, [enclosing()])
        for slot, value in ((5, 1.0e6), (900, 1.0e-6), (2000, 1.0e-6)):
            sizes[slot] = np.float32(value)
            vis.mark_dirty(GV_DIRTY_LOD, slot, 1, pool_id=0)
        fresh = keys_of(True)
        assert gsup.order_of(fresh).tolist() != gsup.order_of(stale).tolist()
        vis.group_draws(0, pool_id=0, by_lod=True)
        gsup.same_records(fetch(vis, n), gsup.expected_results(before, gsup.order_of(fresh)), n)


def run_frame(c, batch, twin):
    s = Setup(c)
    with GpuVisibility(device=0) as vis:
        bind(vis, s.scene)
        vis.bind_geometry(0, s.ids, s.table)
        if batch:
            vis.cull_batch_begin()
        vis.cull(0, [enclosing()])
        vis.group_draws(0, pool_id=0)  # (inside the batch: the recorded cull is launched first)
        if batch:
            vis.cull_batch_end()
        return s, fetch(vis, c.n)


def test_inside_a_cull_batch_and_twice_in_fresh_contexts(twin):
    c = gsup.CASE_BY_NAME["count-2049"]
    s, plain = run_frame(c, False, twin)
    with GpuVisibility(device=0) as vis:
        s.open(vis)
        before = fetch(vis, c.n)
    kappa = gsup.keys(before["visible_idx"], s.ids, c.K)
    gsup.check_conditions(kappa, before["visible_idx"])
    gsup.same_records(plain, gsup.expected_results(before, gsup.order_of(kappa)), c.n)
    _, batched = run_frame(c, True, twin)
    isup.same_results(batched, plain)
    for name in ("count-40000", "K-65536"):  # the same case twice in fresh contexts: identical bytes
        case = gsup.CASE_BY_NAME[name]
        isup.same_results(run_frame(case, False, twin)[1], run_frame(case, False, twin)[1])


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------

def test_error_codes_each_followed_by_a_call_that_succeeds(twin):
    n = 1200
    sc = scene.flat_scene(n, defects=False)
    w = gsup.LodWorld(sc.transforms["position"])
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        lib, ctx = vis.lib, vis.ctx

        def good(by_lod=True):
            vis.bind_geometry(0, w.ids, w.table)
            vis.bind_lod(0, w.sizes, w.lod)
            vis.cull(0, [enclosing()])
            before = fetch(vis, n)
            kappa = gsup.keys(before["visible_idx"], w.ids, len(w.table), (twin, before["baked_model"], w.sizes, 1.0, w.lod) if by_lod else None)
            vis.group_draws(0, pool_id=0, by_lod=by_lod)
            gsup.same_records(fetch(vis, n), gsup.expected_results(before, gsup.order_of(kappa)), n)

        assert lib.gv_pool_group_draws(None, 0, 0, 0, 1.0) == GV_E_ARG                        # a NULL ctx
        vis.bind_geometry(0, w.ids, w.table)
        assert lib.gv_pool_group_draws(ctx, 0, 0, 0, 1.0) == GV_E_ARG                         # no emitted records yet
        good()
        assert lib.gv_pool_group_draws(ctx, 99, 0, 0, 1.0) == GV_E_ARG                        # a pool out of range
        assert lib.gv_pool_group_draws(ctx, 3, 0, 0, 1.0) == GV_E_ARG                         # a pool that is not bound
        assert lib.gv_pool_group_draws(ctx, 0, 0, 2, 1.0) == GV_E_ARG                         # unknown flag bits
        assert lib.gv_pool_group_draws(ctx, 0, 0, GV_GROUP_BY_LOD | 0x80000000, 1.0) == GV_E_ARG
        assert lib.gv_pool_group_draws(ctx, 0, 5, 0, 1.0) == GV_E_ARG                         # a view without emitted records
        good(False)
        vis.cull(0, [enclosing()])
        vis.bind_geometry(0, None, None)
        assert code(vis.group_draws, 0, pool_id=0) == GV_E_STATE                              # no geometry bound
        good()
        vis.cull(0, [enclosing()])
        vis.bind_lod(0, None, None)
        assert code(vis.group_draws, 0, pool_id=0, by_lod=True) == GV_E_STATE                 # the flag without an LOD binding
        vis.group_draws(0, pool_id=0)                                                         # (without the flag it is not needed)
        good()
        vis.cull(0, [enclosing()])
        vis.bind_geometry(0, w.ids[:n - 1], w.table)
        assert code(vis.group_draws, 0, pool_id=0) == GV_E_STATE                              # an id column below the view's occupancy
        vis.bind_geometry(0, w.ids, w.table)
        vis.bind_lod(0, w.sizes[:n - 1], w.lod)
        assert code(vis.group_draws, 0, pool_id=0, by_lod=True) == GV_E_STATE                 # a size column below it
        vis.group_draws(0, pool_id=0)                                                         # (the sizes are not read without the flag)
        good()
        vis.set_instance_layout(0, dtype=isup.BARE)
        vis.emit_instances(0, [0])
        assert code(vis.group_draws, 0, pool_id=0) == GV_E_STATE                              # an instance emission since the last cull
        good()                                                                                # (a new cull ends the emission)


# ---- 7. the drop-in's shim -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def group_commands_driver(tmp_path_factory):
    """tests/cpp/group_commands.cpp, built with the g++ line of tests/test_gpu_lod_select.py"""
    cpp, lib = os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "garden_amd", "lib")
    exe = str(tmp_path_factory.mktemp("group_commands") / "group_commands")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-invalid-offsetof", "-fno-strict-aliasing", "-march=haswell",
                    "-ffp-contract=off", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(cpp, "group_commands.cpp"),
                    "-o", exe, "-L" + lib, "-lgarden_vis", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64",
                    "-lm", "-lpthread"], check=True)
    return exe


def test_group_shim_matches_the_host_loop(group_commands_driver):
    """GpuInstanceWriter + GpuDrawCommands with setGrouping(true) against a host loop that stable-sorts the fetched records by id
    (by id + level for the system with LODs) and writes the same run-mode commands: 30 000 entities, 20 ticks, byte for byte; a
    sorted system throws"""
    p = subprocess.run([group_commands_driver, "--entities", "30000", "--ticks", "20"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["ok"] and out["ticks"] == 20 and out["sorted_throws"] and out["commands"] > 0, out
    assert out["commands"] <= out["geometries"] * out["passes"] * 20, out  # one command per geometry (or level) and pass, not per draw
    assert out["draws"] > 4 * out["commands"], out
