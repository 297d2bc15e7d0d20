"""gv_pool_view_delta on the device: what came into view and what left it since a channel's last call. Expected values are exact:
the oracle's sets of pool slots for the two frames (tests/view_delta_support.py) through np.setdiff1d, compared word for word with
the two lists, which must be in ascending slot order, and with the four counts. tests/test_view_delta_abi.py asserts on the CPU tier
that every case changes between its frames (appeared, vanished and stayed each hold 2 % of the frustum survivors)."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import group_support as gsup
import second_phase_support as sp
import view_delta_support as vd
from garden_amd import scene
from garden_amd.lib import (GV_E_ARG, GV_E_STATE, GV_MAX_DELTA_CHANNELS, GV_MAX_VIEWS, GV_NONE, GV_RESULTS_MAP_VISIBLE, GpuVisibility,
                            GvError)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = np.zeros(0, np.uint32)


def context(c):
    return GpuVisibility(device=0, keep_slot_order=c.keep_slot_order, hiz_rg16f=c.rg16f)


def bind(vis, sc, pool_id=0):
    vis.bind_transforms(sc.transforms, sc.entity_to_transform)
    vis.bind_pool(pool_id, sc.meshes)


def launches(vis):
    return dict(vis.stats()["launches"])


def counted(vis, views, channel=0, restart=False):
    """the call alone, with the launches it added, then the fetch"""
    before = launches(vis)
    vis.view_delta_issue(0, views, channel, restart)
    after = launches(vis)
    return vis.view_delta_fetch(0, channel), {k: after[k] - before[k] for k in after}


def code(fn, *args, **kw):
    with pytest.raises(GvError) as e:
        fn(*args, **kw)
    return e.value.code


def device_words(torch, ptr, count):
    class _Span:
        pass
    span = _Span()
    span.__cuda_array_interface__ = {"shape": (int(count),), "typestr": "<i4", "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(span, device="cuda:0")


def frame(vis, depth, views):
    vis.hiz_build(depth)
    vis.cull(0, views)


# ---- 1. the case table -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sp.CASES, ids=lambda c: c.name)
def test_two_frames_of_the_case_table(case):
    c = case
    first, full = vd.case_sets(c.name)
    a, b = sp.depth_images(c)
    fixed = dict(cull=0, scan=0, emit=3, hiz=0, sweep=0, sort=0)  # one mark launch for the one view, count, place
    with context(c) as vis:
        bind(vis, sp.world(c))
        frame(vis, a, [sp.view()])
        got, added = counted(vis, [0])
        vd.same_answer(got, EMPTY, first, c.n)  # a channel's first call: everything appears, nothing vanishes
        assert added == fixed
        frame(vis, b, [sp.view()])
        got, added = counted(vis, [0])
        vd.same_answer(got, first, full, c.n)
        assert added == fixed
        got, added = counted(vis, [0])          # nothing culled in between: two empty lists, the same |C|
        vd.same_answer(got, full, full, c.n)
        assert added == fixed


# ---- 2. the edges of the new kernels -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", vd.EDGE_SIZES)
def test_edges_of_word_wave_and_workgroup(n):
    c1, c2 = vd.edge_sets(n)
    c3 = vd.enclosed_set(n)
    cam1, cam2 = vd.cameras()
    with GpuVisibility(device=0) as vis:
        bind(vis, vd.edge_world(n))
        for previous, current, view in ((EMPTY, c1, cam1), (c1, c2, cam2), (c2, c3, vd.enclosing()), (c3, c1, cam1)):
            vis.cull(0, [view, dict(view, emit_records=0)])
            vd.same_answer(vis.view_delta(0, [0], channel=0), previous, current, n)  # the records ...
            vd.same_answer(vis.view_delta(0, [1], channel=1), previous, current, n)  # ... and the bytes


# ---- 3. sources --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["flat-4097", "keep-slot-order-4097", "shuffled-4097", "flat-40000", "flat-100003"])
def test_count_only_main_view_answers_like_the_emitted_view(name):
    """the bytes through the entry -> slot table (a mirror in spatial order) and as ballot words (GV_CONFIG_KEEP_SLOT_ORDER)"""
    c = sp.CASE_BY_NAME[name]
    first, full = vd.case_sets(name)
    a, b = sp.depth_images(c)
    views = [sp.view(), dict(sp.view(), emit_records=0)]
    with context(c) as vis:
        bind(vis, sp.world(c))
        permuted = (np.diff(vis.mirror_slots(0, c.n).astype(np.int64)) < 0).any()
        assert permuted != c.keep_slot_order
        frame(vis, a, views)
        vd.same_answer(vis.view_delta(0, [1], channel=2), EMPTY, first, c.n)
        frame(vis, b, views)
        vd.same_answer(vis.view_delta(0, [1], channel=2), first, full, c.n)
        vd.same_answer(vis.view_delta(0, [0], channel=0), EMPTY, full, c.n)
        vd.same_answer(vis.view_delta(0, [0, 1], channel=3), EMPTY, full, c.n)  # both sources in one call: the same set


def test_count_only_shadow_view_is_refused():
    c = sp.CASE_BY_NAME["flat-257"]
    with context(c) as vis:
        bind(vis, sp.world(c))
        vis.cull(0, [scene.main_camera_view(), dict(scene.cascade_view(index=0), emit_records=0)])
        assert code(vis.view_delta_issue, 0, [1]) == GV_E_STATE
        assert code(vis.view_delta_issue, 0, [0, 1]) == GV_E_STATE
        assert code(vis.view_delta_fetch, 0) == GV_E_STATE  # the refused calls left no result
        vis.view_delta(0, [0])


# ---- 4. union ----------------------------------------------------------------------------------------------------------------------

def test_main_pass_and_a_cascade_give_the_union():
    c = sp.CASE_BY_NAME["flat-40000"]
    sc = sp.world(c)
    main, cascade = scene.main_camera_view(), scene.cascade_view(index=0)
    in_main, in_cascade = vd.slots_of(sc, main), vd.slots_of(sc, cascade)
    assert len(np.setdiff1d(in_main, in_cascade)) and len(np.setdiff1d(in_cascade, in_main)) and len(np.intersect1d(in_main, in_cascade))
    with context(c) as vis:
        bind(vis, sc)
        vis.cull(0, [main, cascade])
        vd.same_answer(vis.view_delta(0, [1], channel=1), EMPTY, in_cascade, c.n)
        vd.same_answer(vis.view_delta(0, [1, 0], channel=0), EMPTY, np.union1d(in_main, in_cascade), c.n)
        vis.cull(0, [main, cascade])
        vd.same_answer(vis.view_delta(0, [0], channel=0), np.union1d(in_main, in_cascade), in_main, c.n)


@pytest.mark.parametrize("name", ["flat-4097", "flat-100003"])
def test_both_views_of_a_two_phase_frame_give_the_second_views_bytes(name):
    c, e = sp.CASE_BY_NAME[name], sp.expected(name)
    a, b = sp.depth_images(c)
    with context(c) as vis:
        bind(vis, sp.world(c))
        frame(vis, a, [sp.view()])
        vis.hiz_build(b)
        vis.cull_second_phase(0, 1, sp.view(), pool_id=0)
        union = vis.view_delta(0, [0, 1], channel=0)
        alone = vis.view_delta(0, [1], channel=1)
        fetched = vis.fetch(1, write_back=False, occupancy=c.n, pool_id=0)
        assert union["appeared"].tolist() == np.flatnonzero(fetched["is_visible"]).tolist() == np.flatnonzero(e.second["is_visible"]).tolist()
        assert alone["appeared"].tolist() == fetched["visible_idx"].tolist() == e.second["visible_idx"].tolist()
        assert union["visible_count"] == int(e.second["is_visible"].sum()) and alone["visible_count"] == e.second["draw_count"]


# ---- 5. order and state independence -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["sort", "sort-descending", "grouped", "batch"])
def test_same_answer_whatever_order_the_records_are_in(how):
    c = sp.CASE_BY_NAME["flat-40000"]
    first, full = vd.case_sets(c.name)
    a, b = sp.depth_images(c)
    with context(c) as vis:
        bind(vis, sp.world(c))
        if how == "grouped":
            ids = np.random.Generator(np.random.PCG64(c.n)).integers(0, 12, c.n).astype(np.uint32)
            vis.bind_geometry(0, ids, gsup.geometry_table(12))
        for previous, current, depth in ((EMPTY, first, a), (first, full, b)):
            vis.hiz_build(depth)
            if how == "batch":
                vis.cull_batch_begin()
            vis.cull(0, [sp.view()])
            if "sort" in how:
                vis.sort(0, descending=(how == "sort-descending"), pool_id=0)
            if how == "grouped":
                vis.group_draws(0, pool_id=0)
            vd.same_answer(vis.view_delta(0, [0]), previous, current, c.n)
            raw = vis.fetch(0, write_back=False, occupancy=c.n, order="raw", pool_id=0)
            assert (np.diff(raw["visible_idx"].astype(np.int64)) < 0).any()  # the records are NOT in slot order
            assert np.sort(raw["visible_idx"]).tolist() == current.tolist()


def test_the_call_changes_nothing_another_call_can_observe():
    import bounds_support as bs
    import instances_support as isup
    c = sp.CASE_BY_NAME["flat-40000"]
    a, _ = sp.depth_images(c)
    views = [sp.view(), dict(sp.view(), emit_records=0)]
    ids = np.random.Generator(np.random.PCG64(c.n)).integers(0, 12, c.n).astype(np.uint32)
    commands = np.dtype([("count", np.uint32), ("instance_count", np.uint32), ("first", np.uint32), ("first_instance", np.uint32)])
    with context(c) as vis:
        bind(vis, sp.world(c))
        vis.bind_geometry(0, ids, gsup.geometry_table(12))
        vis.set_instance_layout(0, dtype=isup.FULL)
        vis.set_command_layout(0, dtype=commands)
        frame(vis, a, views)
        vis.emit_instances(0, [0])
        vis.emit_draw_commands(0)
        vis.view_bounds_issue(0, [0], bs.IDENTITY)
        before = [vis.fetch(v, write_back=False, occupancy=c.n, order="raw", pool_id=0) for v in (0, 1)]
        made = (vis.instances(0), vis.draw_commands(0), vis.view_bounds_fetch(0))
        vis.view_delta(0, [0], channel=0)
        vis.view_delta(0, [1], channel=1)
        vis.view_delta(0, [0, 1], channel=2, restart=True)
        for v in (0, 1):
            isup.same_results(vis.fetch(v, write_back=False, occupancy=c.n, order="raw", pool_id=0), before[v])
        again = (vis.instances(0), vis.draw_commands(0), vis.view_bounds_fetch(0))
        for was, now in zip(made[:2], again[:2]):
            assert was[0].tobytes() == now[0].tobytes() and was[1].tolist() == now[1].tolist() and len(was[0])
        assert made[2].tobytes() == again[2].tobytes()


def test_growth_churn_and_a_reordered_mirror_between_two_calls():
    """the pool grows step by step (every step appends slots; the mirror is re-ordered on the way), entities move through dirty
    marks: the baseline is slot numbers, so the next call differs from the set of the LAST call whatever happened to the mirror.
    New slots can only appear."""
    from garden_amd.lib import GV_DIRTY_TRANSFORM
    full = scene.flat_scene(260_000, seed=vd.SEED + 5)
    cam1, cam2 = vd.cameras()

    def cut(k):
        e2t = full.entity_to_transform.copy()
        e2t[e2t >= k] = GV_NONE
        return scene.Scene(full.meshes[:k].copy(), full.transforms[:k].copy(), e2t)

    with GpuVisibility(device=0, linear_scan=True) as vis:
        sc = cut(150_000)
        bind(vis, sc)
        vis.cull(0, [cam1])
        c1 = vd.slots_of(sc, cam1)
        vd.same_answer(vis.view_delta(0, [0]), EMPTY, c1, 150_000)
        reorders = vis.stats()["mirror_reorders"]
        for k in (160_000, 175_000, 200_000, 230_000, 260_000):
            sc = cut(k)
            bind(vis, sc)
            vis.cull(0, [cam1])
        assert vis.stats()["mirror_reorders"] > reorders
        sc.transforms["position"][1000:1400, :3] += np.float32(25.0)
        vis.mark_dirty(GV_DIRTY_TRANSFORM, 1000, 400)
        vis.cull(0, [cam2])
        c2 = vd.slots_of(sc, cam2)
        got = vis.view_delta(0, [0])
        vd.same_answer(got, c1, c2, 260_000)
        assert (got["appeared"] >= 150_000).any() and (got["vanished"] < 150_000).all()


# ---- 6. universe -------------------------------------------------------------------------------------------------------------------

def test_a_pool_that_shrank_loses_the_slots_beyond_its_occupancy():
    n, fewer = 2 * vd.GROUP + 1, vd.GROUP + vd.WORD + 3
    sc = vd.edge_world(n)
    cam1, _ = vd.cameras()
    c1 = vd.edge_sets(n)[0]
    small = scene.Scene(sc.meshes[:fewer].copy(), sc.transforms, sc.entity_to_transform)
    c2 = vd.slots_of(small, cam1)
    assert c2.tolist() == c1[c1 < fewer].tolist() and (c1 >= fewer).any()
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.cull(0, [cam1])
        vd.same_answer(vis.view_delta(0, [0]), EMPTY, c1, n)
        vis.bind_pool(0, small.meshes)
        vis.cull(0, [cam1])
        vd.same_answer(vis.view_delta(0, [0]), c1, c2, n)       # U = max(P.slots, C.slots): what lay beyond has vanished
        vd.same_answer(vis.view_delta(0, [0]), c2, c2, fewer)   # ... and the baseline covers the new occupancy only
        vis.bind_pool(0, sc.meshes)
        vis.cull(0, [cam1])
        got = vis.view_delta(0, [0])
        vd.same_answer(got, c2, c1, n)                          # grown again: the new slots can only appear
        assert len(got["vanished"]) == 0 and (got["appeared"] >= fewer).all()


# ---- 7. channels, restart, drop ----------------------------------------------------------------------------------------------------

def test_channels_restart_and_drop():
    n = vd.WAVE + 1
    c1, c2 = vd.edge_sets(n)
    c3 = vd.enclosed_set(n)
    cam1, cam2 = vd.cameras()
    with GpuVisibility(device=0) as vis:
        bind(vis, vd.edge_world(n))
        vis.cull(0, [cam1, cam2])
        vd.same_answer(vis.view_delta(0, [0], channel=0), EMPTY, c1, n)
        vd.same_answer(vis.view_delta(0, [1], channel=GV_MAX_DELTA_CHANNELS - 1), EMPTY, c2, n)
        vis.cull(0, [cam2, vd.enclosing()])
        vd.same_answer(vis.view_delta(0, [0], channel=0), c1, c2, n)  # each channel against ITS baseline
        vd.same_answer(vis.view_delta(0, [1], channel=GV_MAX_DELTA_CHANNELS - 1), c2, c3, n)
        vd.same_answer(vis.view_delta_fetch(0, channel=0), c1, c2, n)  # ... and its answer is still there behind the other's call
        vd.same_answer(vis.view_delta(0, [0], channel=0, restart=True), EMPTY, c2, n)
        vd.same_answer(vis.view_delta(0, [1], channel=0), c2, c3, n)  # the restart committed like any call
        vis.view_delta_drop(0, channel=0)
        assert code(vis.view_delta_fetch, 0, 0) == GV_E_STATE and code(vis.view_delta_device, 0, 0) == GV_E_STATE
        vd.same_answer(vis.view_delta_fetch(0, channel=GV_MAX_DELTA_CHANNELS - 1), c2, c3, n)
        vd.same_answer(vis.view_delta(0, [1], channel=0), EMPTY, c3, n)  # behind a drop: a first call
        vd.same_answer(vis.view_delta(0, [0], channel=GV_MAX_DELTA_CHANNELS - 1), c3, c2, n)


# ---- 8. write-back -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["flat-4097", "flat-100003"])
def test_write_back_touches_the_listed_bytes_only(name):
    c = sp.CASE_BY_NAME[name]
    first, full = vd.case_sets(name)
    a, b = sp.depth_images(c)
    sc = sp.world(c)
    stays = int(np.intersect1d(first, full)[0])  # a slot whose byte does not change between the frames
    with context(c) as vis:
        bind(vis, sc)
        frame(vis, a, [sp.view()])
        vis.view_delta(0, [0])
        sc.meshes["isVisible"] = vd.bytes_of(first, c.n)  # the caller's bytes hold the baseline ...
        sc.meshes["isVisible"][stays] = 7                 # ... and a mark where nothing may be written
        frame(vis, b, [sp.view()])
        got = vis.view_delta(0, [0], write_back=True)
        vd.same_answer(got, first, full, c.n)
        want = vd.bytes_of(full, c.n)
        want[stays] = 7
        assert sc.meshes["isVisible"].tolist() == want.tolist()


def test_write_back_through_the_result_mapping_with_holes():
    c = sp.CASE_BY_NAME["flat-4097"]
    first, full = vd.case_sets(c.name)
    a, b = sp.depth_images(c)
    sc = sp.world(c)
    rng = np.random.Generator(np.random.PCG64(c.n))
    world_slots = c.n + 100
    table = rng.permutation(world_slots)[:c.n].astype(np.uint32)
    holes = rng.random(c.n) < 0.1
    table[holes] = GV_NONE
    beyond = np.flatnonzero(~holes)[::50]
    table[beyond] = world_slots + 5  # past visible_count: skipped like a hole
    mapped = ~holes & (table < world_slots)
    assert holes[first].any() and holes[full].any() and (~mapped[np.setdiff1d(full, first)]).any() and mapped[np.setdiff1d(first, full)].any()
    world = np.full(world_slots * 2, 9, np.uint8)  # stride 2: the odd bytes are never the library's

    def expected(slots):
        out = world.copy()
        out[::2] = 9
        live = np.flatnonzero(mapped)
        out[table[live].astype(np.int64) * 2] = vd.bytes_of(slots, c.n)[live]
        return out

    with context(c) as vis:
        bind(vis, sc)
        vis.set_index_map(0, table)
        vis.set_result_mapping(0, GV_RESULTS_MAP_VISIBLE, world, stride=2)
        frame(vis, a, [sp.view()])
        vis.view_delta(0, [0])
        world[:] = expected(first)
        sc.meshes["isVisible"] = 5
        frame(vis, b, [sp.view()])
        vd.same_answer(vis.view_delta(0, [0], write_back=True), first, full, c.n)  # the lists are pool slots, never mapped
        assert world.tolist() == expected(full).tolist()
        assert (sc.meshes["isVisible"] == 5).all()  # the bound column is not the target


# ---- 9. the device pointers --------------------------------------------------------------------------------------------------------

def test_device_pointers_hold_what_the_fetch_delivers():
    import torch
    n = vd.GROUP + 1
    c1, c2 = vd.edge_sets(n)
    cam1, cam2 = vd.cameras()
    with GpuVisibility(device=0) as vis:
        bind(vis, vd.edge_world(n))
        vis.cull(0, [cam1])
        vis.view_delta(0, [0])
        vis.cull(0, [cam2])
        vis.view_delta_issue(0, [0])
        slots, counts = vis.view_delta_device(0)
        vis.wait()
        four = device_words(torch, counts, 4).cpu().numpy().view(np.uint32)
        appeared, vanished = vd.delta(c1, c2)
        assert four.tolist() == [len(appeared), len(vanished), len(c2), n]
        words = device_words(torch, slots, len(appeared) + len(vanished)).cpu().numpy().view(np.uint32)
        assert words.tolist() == appeared.tolist() + vanished.tolist()
        vd.same_answer(vis.view_delta_fetch(0), c1, c2, n)


# ---- 10. errors --------------------------------------------------------------------------------------------------------------------

def test_errors():
    c = sp.CASE_BY_NAME["flat-257"]
    sc = sp.world(c)
    main = scene.main_camera_view()
    with context(c) as vis:
        lib = vis.lib
        assert lib.gv_pool_view_delta(None, 0, 0, None, 0, 0) == GV_E_ARG
        assert lib.gv_pool_view_delta_device(None, 0, 0, None, None) == GV_E_ARG
        assert lib.gv_pool_view_delta_fetch(None, 0, 0, 0, None) == GV_E_ARG
        assert code(vis.view_delta_issue, 0, [0]) == GV_E_ARG                      # a pool that is not bound
        bind(vis, sc)
        assert code(vis.view_delta_issue, 0, [0]) == GV_E_ARG                      # no cull of the pool ever had a view there
        vis.cull(0, [main, main, dict(main, emit_records=0)])
        assert code(vis.view_delta_issue, 99, [0]) == GV_E_ARG
        assert code(vis.view_delta_issue, 0, [0], GV_MAX_DELTA_CHANNELS) == GV_E_ARG
        assert code(vis.view_delta_drop, 0, GV_MAX_DELTA_CHANNELS) == GV_E_ARG
        assert code(vis.view_delta_issue, 0, list(range(GV_MAX_VIEWS)) + [0]) == GV_E_ARG
        assert code(vis.view_delta_issue, 0, [GV_MAX_VIEWS]) == GV_E_ARG
        assert code(vis.view_delta_issue, 0, [0, 1, 0]) == GV_E_ARG                # listed twice
        assert code(vis.view_delta_issue, 0, [0, 5]) == GV_E_ARG                   # never a view
        idx = (ctypes.c_uint32 * 1)(0)
        assert lib.gv_pool_view_delta(vis.ctx, 0, 0, idx, 1, 2) == GV_E_ARG        # unknown flag bits
        assert lib.gv_pool_view_delta(vis.ctx, 0, 0, None, 1, 0) == GV_E_ARG       # NULL views with a count
        assert code(vis.view_delta_fetch, 0, 0) == GV_E_STATE                      # every refusal left the channel without a result
        assert code(vis.view_delta_device, 0, 1) == GV_E_STATE
        assert code(vis.view_delta_fetch, 0, GV_MAX_DELTA_CHANNELS) == GV_E_ARG
        assert code(vis.view_delta_device, 99, 0) == GV_E_ARG
        first = vis.view_delta(0, [0, 2])
        assert lib.gv_pool_view_delta_fetch(vis.ctx, 0, 0, 0, None) == GV_E_ARG
        assert lib.gv_pool_view_delta_device(vis.ctx, 0, 0, None, None) == GV_E_ARG
        vis.cull(0, [main])                                                        # a narrower cull: views 1 and 2 have no results
        assert code(vis.view_delta_issue, 0, [0, 2]) == GV_E_STATE
        assert code(vis.view_delta_issue, 0, [1]) == GV_E_STATE
        again = vis.view_delta_fetch(0)                                            # a failed call changes nothing: the answer ...
        assert again["appeared"].tolist() == first["appeared"].tolist() and again["visible_count"] == first["visible_count"] > 0
        got = vis.view_delta(0, [0])                                               # ... and the baseline
        assert len(got["appeared"]) == len(got["vanished"]) == 0 and got["visible_count"] == first["visible_count"]
    with context(c) as vis:  # write_back without a target: columns bound without an isVisible array
        vis.bind_transforms(sc.transforms, sc.entity_to_transform)
        columns = dict(entity=sc.meshes["entity"], is_enabled=sc.meshes["isEnabled"], aabb_min=sc.meshes["aabbMin"], aabb_max=sc.meshes["aabbMax"])
        vis.bind_pool_columns(0, columns)
        vis.cull(0, [main])
        vis.view_delta_issue(0, [0])
        assert code(vis.view_delta_fetch, 0, 0, True) == GV_E_STATE
        assert vis.view_delta_fetch(0, 0)["visible_count"] > 0


def test_an_empty_pool_and_a_view_without_draws_are_ok():
    sc = scene.flat_scene(8, seed=sp.SEED)
    nothing = scene.make_view(scene.ortho_rev_z(10.0, 10.0, -5.0, 5.0), camera_position=(1.0e9, 0.0, 0.0))
    with GpuVisibility(device=0) as vis:
        vis.bind_transforms(sc.transforms, sc.entity_to_transform)
        vis.bind_pool(0, sc.meshes[:0])
        vis.cull(0, [scene.main_camera_view()])
        vd.same_answer(vis.view_delta(0, [0]), EMPTY, EMPTY, 0)
        vis.bind_pool(0, sc.meshes)
        vis.cull(0, [nothing, dict(nothing, emit_records=0)])
        vd.same_answer(vis.view_delta(0, [0, 1]), EMPTY, EMPTY, 8)


# ---- 11. the drivers ---------------------------------------------------------------------------------------------------------------

def test_shim_driver():
    """tests/cpp/view_delta.cpp: GpuVisibleDelta::writeBack against the CPU system's isVisible bytes on every tick of a camera that
    steps, and its appeared / vanished spans against a host loop over two consecutive frames' bytes"""
    exe = os.path.join(ROOT, "tests", "cpp", "build", "view_delta")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "view_delta.mk"], check=True)
    out = subprocess.run([exe, "--entities", "10000", "--ticks", "8"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "view_delta ok" in out.stdout
    report = json.loads(out.stdout.strip().splitlines()[0])
    assert report["ok"] and report["ticks"] == 8 and min(report["appeared"], report["vanished"]) > 0 and report["full_write_backs"] >= 1, report
