"""gv_pool_view_bounds on the device: the bounds of a view's visible draws in a caller's basis. Expected values come from the C twin
of the rule (tests/bounds_twin.h) applied to the records FETCHED in front of the call and the boxes of their pool slots, and are
exact: every one of the 8 words of every item. The sizes come from tests/bounds_support.py, which reads the records per workgroup
and the workgroup size from the kernel header; the conditions that keep a case from passing by accident are asserted on the oracle
by tests/test_bounds_abi.py and, where the device's own records decide, again here."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import bounds_support as bs
import commands_support as csup
import instances_support as isup
import lod_support as lsup
import second_phase_support as sp
from garden_amd import scene
from garden_amd.lib import (GV_DIRTY_TRANSFORM, GV_E_ARG, GV_E_STATE, GV_MAX_BOUNDS_ITEMS, GV_MAX_VIEWS, GpuVisibility, GvError,
                            GvViewBounds)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return bs.build_twin(tmp_path_factory.mktemp("bounds_twin"))


def bind(vis, sc, pool_id=0):
    vis.bind_transforms(sc.transforms, sc.entity_to_transform)
    vis.bind_pool(pool_id, sc.meshes)
    vis.hierarchy_rebuild()


def fetch(vis, view, occupancy, pool_id=0):
    return vis.fetch(view, write_back=False, occupancy=occupancy, order="raw", pool_id=pool_id)


def code(fn, *args, **kw):
    with pytest.raises(GvError) as e:
        fn(*args, **kw)
    return e.value.code


def check(vis, twin, views, bases, boxes, occupancy, pool_id=0):
    """Fetches the listed views, issues ONE call for all items and compares every word of every item with the twin over the fetched
    records. Returns (the bounds, the fetched results by view)."""
    fetched = {v: fetch(vis, v, occupancy, pool_id) for v in set(views)}
    exp = np.array([bs.expected(twin, fetched[v], boxes, b) for v, b in zip(views, bases)], bs.BOUNDS_DTYPE)
    got = vis.view_bounds(pool_id, views, bases)
    assert len(got) == len(views)
    assert bs.words(got) == bs.words(exp)
    for item, v in zip(got, views):
        assert int(item["draw_count"]) == int(fetched[v]["draw_count"])
    return got, fetched


# ---- 1. parity at lane, wave, workgroup and partial-row edges -----------------------------------------------------------------------

@pytest.mark.parametrize("n", bs.EDGE_SIZES)
def test_every_word_equals_the_twin_at_the_edges(n, twin):
    """an enclosing frustum: n visible records == the pool size; a random rotation basis with a translation"""
    sc = bs.edge_world(n)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.cull(0, [bs.enclosing()])
        got, fetched = check(vis, twin, [0], [bs.rotation_basis(n, (3.5, -20.0, 100.0))], bs.aabbs_by_slot(sc.meshes), n)
        assert int(fetched[0]["draw_count"]) == n == int(got[0]["draw_count"]) and int(got[0]["nan_records"]) == 0
        if n > 64:
            assert fetched[0]["visible_idx"][:n].tolist() != list(range(n))  # (the mirror's own order is in play)
        assert (got[0]["lo"] < got[0]["hi"]).all()


# ---- 2. the outlier sweep ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis,side", [(a, s) for a in range(3) for s in (-1, 1)])
def test_an_outlier_at_any_delivery_position_is_found(axis, side, twin):
    """2R + 1 records; the record at delivery position k is pushed far out along one axis: a dropped lane, wave, workgroup or
    partial row loses it"""
    n = bs.OUTLIER_WORLD
    sc = bs.edge_world(n)
    boxes = bs.aabbs_by_slot(sc.meshes)
    position = sc.transforms["position"]
    far = np.float32(side * 1.0e5)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.cull(0, [bs.enclosing()])
        order = fetch(vis, 0, n)["visible_idx"][:n].copy()
        plain = vis.view_bounds(0, [0], [bs.IDENTITY])[0]
        assert abs(float(plain["lo"][axis])) < 2.0e3 and abs(float(plain["hi"][axis])) < 2.0e3
        for k in bs.OUTLIER_POSITIONS:
            slot = int(order[k])
            kept = position[slot, axis].copy()
            position[slot, axis] = far
            vis.mark_dirty(GV_DIRTY_TRANSFORM, slot, 1)
            vis.cull(0, [bs.enclosing()])
            got, fetched = check(vis, twin, [0], [bs.IDENTITY], boxes, n)
            assert int(fetched[0]["visible_idx"][k]) == slot and int(got[0]["draw_count"]) == n  # (the mirror kept its order)
            value = float(got[0]["hi" if side > 0 else "lo"][axis])
            assert abs(value - float(far)) < 10.0, (k, value)
            other = float(got[0]["lo" if side > 0 else "hi"][axis])
            assert abs(other) < 2.0e3
            position[slot, axis] = kept
            vis.mark_dirty(GV_DIRTY_TRANSFORM, slot, 1)


# ---- 3. order and state independence -------------------------------------------------------------------------------------------------

def test_same_bounds_in_morton_and_slot_order_and_after_sort_and_grouping(twin):
    n = 5000
    sc = scene.flat_scene(n, seed=scene.SEED + 31)
    boxes = bs.aabbs_by_slot(sc.meshes)
    bases = [bs.rotation_basis(5), bs.IDENTITY]
    answers = []
    for keep_slot_order in (False, True):
        with GpuVisibility(device=0, keep_slot_order=keep_slot_order) as vis:
            bind(vis, sc)
            vis.cull(0, [bs.enclosing()])
            got, fetched = check(vis, twin, [0, 0], bases, boxes, n)
            draws = int(fetched[0]["draw_count"])
            assert 0.9 * n < draws < n  # (the world's defects are not drawn)
            ascending = (np.diff(fetched[0]["visible_idx"][:draws].astype(np.int64)) > 0).all()
            assert ascending == keep_slot_order
            answers.append(bs.words(got))
            if keep_slot_order:
                continue
            unsorted = fetched[0]["visible_idx"][:draws].copy()
            for descending in (False, True):
                vis.sort(0, descending=descending, pool_id=0)
                got, fetched = check(vis, twin, [0, 0], bases, boxes, n)  # (the fetch in front launches the deferred sort)
                assert fetched[0]["visible_idx"][:draws].tolist() != unsorted.tolist()
                answers.append(bs.words(got))
                vis.sort(0, descending=not descending, pool_id=0)  # ... and here the call itself does
                answers.append(bs.words(vis.view_bounds(0, [0, 0], bases)))
            ids = np.random.Generator(np.random.PCG64(n)).integers(0, 12, n).astype(np.uint32)
            vis.bind_geometry(0, ids, csup.geometry_table([(3 * (g + 1), 100 * g, g) for g in range(12)]))
            vis.cull(0, [bs.enclosing()])
            vis.group_draws(0, pool_id=0)
            got, fetched = check(vis, twin, [0, 0], bases, boxes, n)
            grouped = ids[fetched[0]["visible_idx"][:draws]]
            assert (np.diff(grouped.astype(np.int64)) >= 0).all() and fetched[0]["visible_idx"][:draws].tolist() != unsorted.tolist()
            answers.append(bs.words(got))
    assert all(a == answers[0] for a in answers)


def test_a_second_phase_view(twin):
    c = sp.CASE_BY_NAME["flat-4097"]
    a, b = sp.depth_images(c)
    sc = sp.world(c)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.hiz_build(a)
        vis.cull(0, [sp.view()])
        vis.hiz_build(b)
        vis.cull_second_phase(0, 1, sp.view(), pool_id=0)
        got, fetched = check(vis, twin, [0, 1, 1], [bs.rotation_basis(2), bs.rotation_basis(2), bs.IDENTITY], bs.aabbs_by_slot(sc.meshes), c.n)
        first, second = int(fetched[0]["draw_count"]), int(fetched[1]["draw_count"])
        assert first > 16 and second > 16 and not np.isin(fetched[1]["visible_idx"][:second], fetched[0]["visible_idx"][:first]).any()
        assert bs.words(got[:1]) != bs.words(got[1:2])
        # the second phase ends the pool's result like a cull
        vis.cull_second_phase(0, 1, sp.view(), pool_id=0)
        assert code(vis.view_bounds_fetch, 0) == GV_E_STATE


def test_a_pool_with_a_hierarchy_takes_the_chain_from_the_records(twin):
    n = 6000
    sc = scene.hierarchy_scene(n, depth=4, seed=scene.SEED + 33)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.cull(0, [bs.enclosing()])
        got, fetched = check(vis, twin, [0], [bs.rotation_basis(3)], bs.aabbs_by_slot(sc.meshes), n)
        draws = int(fetched[0]["draw_count"])
        assert draws > 0.8 * n
        # (the records' translations are not the entities' own positions: the chain is in bakedModel)
        models = fetched[0]["baked_model"].reshape(-1, 12)[:draws]
        own = sc.transforms["position"][fetched[0]["visible_idx"][:draws], :3]
        assert (np.abs(models[:, 9:12] - own).max(axis=1) > 1.0).sum() > draws // 2


def test_a_pool_with_an_index_map_is_read_by_pool_slot(twin):
    n = 3000
    sc = scene.flat_scene(n, seed=scene.SEED + 34, defects=False)
    boxes = bs.aabbs_by_slot(sc.meshes)
    basis = bs.rotation_basis(4)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.cull(0, [bs.enclosing()])
        plain, _ = check(vis, twin, [0], [basis], boxes, n)
        # a map that reverses the slots and reaches beyond the pool: a kernel that looked boxes up by mapped slot would read elsewhere
        vis.set_index_map(0, (np.arange(n, dtype=np.uint32)[::-1] + 7).copy())
        vis.cull(0, [bs.enclosing()])
        mapped, fetched = check(vis, twin, [0], [basis], boxes, n)
        assert int(fetched[0]["visible_idx"][:n].max()) == n - 1  # (records hold POOL slots)
        assert bs.words(mapped) == bs.words(plain)


# ---- 4. items ------------------------------------------------------------------------------------------------------------------------

def test_eight_items_over_three_views_equal_eight_single_calls(twin):
    n = 3000
    sc = scene.flat_scene(n, seed=scene.SEED + 35)
    boxes = bs.aabbs_by_slot(sc.meshes)
    side = 100.0 * n ** (1.0 / 3.0)
    part = scene.make_view(scene.ortho_rev_z(0.7 * side, 0.7 * side, -side, side), shadow_pass=1)
    views = [bs.enclosing(), bs.enclosing(shadow_pass=0, camera_offset=(3.5, -2.0, 1.25)), part]
    a, b, c = bs.rotation_basis(6), bs.rotation_basis(7, (1.0, 2.0, 3.0)), bs.rotation_basis(8, (-50.0, 0.25, 9.0))
    items = [(0, a), (0, b), (1, a), (1, c), (2, a), (2, bs.IDENTITY), (1, bs.IDENTITY), (0, bs.extreme_basis())]
    assert len(items) == GV_MAX_BOUNDS_ITEMS
    listed, bases = [v for v, _ in items], [m for _, m in items]
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.cull(0, views)
        got, fetched = check(vis, twin, listed, bases, boxes, n)
        seen = [int(fetched[v]["draw_count"]) for v in range(3)]
        assert seen[0] == seen[1] > 0.9 * n and 100 < seen[2] < seen[0] - 100
        # the shadow pass shares the camera position: its records' models are the main view's, camera_offset does not enter
        assert bs.words(got[2:3]) == bs.words(got[0:1]) and bs.words(got[0:1]) != bs.words(got[1:2])
        assert (got[4]["lo"] >= got[0]["lo"]).all() and (got[4]["hi"] <= got[0]["hi"]).all() and bs.words(got[4:5]) != bs.words(got[0:1])
        pointer, count = vis.view_bounds_device(0)
        assert pointer and count == 8
        singles = [vis.view_bounds(0, [v], [m])[0] for v, m in items]
        assert vis.view_bounds_device(0)[1] == 1
        assert bs.words(np.array(singles, bs.BOUNDS_DTYPE)) == bs.words(got)


# ---- 5. planted extremes -------------------------------------------------------------------------------------------------------------

def test_planted_extremes_in_models_and_in_the_basis(twin):
    sc, planted = bs.planted_world()
    n = bs.PLANTED_N
    boxes = bs.aabbs_by_slot(sc.meshes)
    bases = [bs.rotation_basis(0), bs.IDENTITY, bs.extreme_basis()]
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.cull(0, [bs.enclosing(bs.PLANTED_HALF)])
        got, fetched = check(vis, twin, [0, 0, 0], bases, boxes, n)
        draws = int(fetched[0]["draw_count"])
        assert draws > 0.9 * n and np.isin(planted, fetched[0]["visible_idx"][:draws]).sum() > 0.9 * len(planted)
        nan_records = int(got[0]["nan_records"])
        assert 0 < nan_records < bs.NAN_CAP * draws
        assert nan_records == int(bs.expected(twin, fetched[0], boxes, bases[0])["nan_records"])
        assert np.isinf(got[0]["lo"]).any() or np.isinf(got[0]["hi"]).any()          # infinities took part
        assert np.isfinite(got[1]["lo"]).all() and np.abs(got[1]["lo"]).max() > 1e19  # the far pivots are the identity's extremes
        assert float(got[2]["lo"][2]) == np.inf and float(got[2]["hi"][2]) == -np.inf and int(got[2]["nan_records"]) == draws
        assert float(got[2]["lo"][0]) == -np.inf and float(got[2]["hi"][0]) == np.inf


# ---- 6. nothing else moves -----------------------------------------------------------------------------------------------------------

def test_nothing_else_moves_launches_are_counted_and_the_result_ends_with_the_cull(twin):
    n = 5000
    sc = scene.flat_scene(n, seed=scene.SEED + 36)
    rng = np.random.Generator(np.random.PCG64(36))
    ids = (rng.integers(0, 2, n) * 2).astype(np.uint32)
    sizes = rng.uniform(0.5, 4.0, n).astype(np.float32)
    table = csup.geometry_table([(6, 0, 0), (9, 6, 1), (12, 15, 2), (15, 27, 3)])
    lod = lsup.lod_table([(2, [300.0]), (1, []), (2, [500.0]), (1, [])])
    views = [bs.enclosing(), scene.cascade_view(index=0, size=400.0)]
    bases = [bs.rotation_basis(10), bs.rotation_basis(11), bs.IDENTITY]
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_geometry(0, ids, table)
        vis.bind_lod(0, sizes, lod)
        vis.cull(0, views)
        vis.sort(1, pool_id=0)
        vis.set_instance_layout(0, dtype=isup.FULL)
        vis.emit_instances(0, [0, 1])
        vis.select_lods(0, [1.0, 0.5])
        vis.set_command_layout(0, dtype=csup.INDEXED)
        vis.emit_draw_commands(0, merge_runs=True)

        def everything():
            results = [fetch(vis, v, n) for v in (0, 1)]
            instances, starts = vis.instances(0)
            g, counts = vis.lods(0)
            commands, command_counts = vis.draw_commands(0)
            return results, (instances.tobytes(), starts.tobytes(), [x.tobytes() for x in g], counts.tobytes(), commands.tobytes(),
                             command_counts.tobytes())

        before_results, before_rest = everything()
        assert before_results[0]["is_visible"] is not None and int(before_results[1]["draw_count"]) > 0
        stats = vis.stats()
        for _ in range(2):
            vis.view_bounds_issue(0, [0, 1, 0], bases)
        after = vis.stats()
        grown = {k: after["launches"][k] - stats["launches"][k] for k in after["launches"]}
        assert grown.pop("emit") == 4 and not any(grown.values()), grown  # two launches per call, nothing else
        assert after["upload_bytes"] == stats["upload_bytes"]
        check(vis, twin, [0, 1, 0], bases, bs.aabbs_by_slot(sc.meshes), n)
        after_results, after_rest = everything()
        for x, y in zip(before_results, after_results):
            isup.same_results(x, y)
        assert before_rest == after_rest
        # the result is the pool's until its next cull
        assert len(vis.view_bounds_fetch(0)) == 3
        vis.cull(0, views)
        assert code(vis.view_bounds_fetch, 0) == GV_E_STATE and code(vis.view_bounds_device, 0) == GV_E_STATE


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------------

def test_error_codes_each_followed_by_a_correct_call(twin):
    n = 1200
    sc = scene.flat_scene(n, seed=scene.SEED + 37)
    boxes = bs.aabbs_by_slot(sc.meshes)
    nothing = scene.make_view(scene.ortho_rev_z(10.0, 10.0, -5.0, 5.0), camera_position=(1.0e6, 0.0, 0.0), shadow_pass=1)
    count_only = bs.enclosing(shadow_pass=2)
    count_only["emit_records"] = 0
    views = [bs.enclosing(), nothing, count_only]
    basis = bs.rotation_basis(12)
    with GpuVisibility(device=0) as vis:
        lib, ctx = vis.lib, vis.ctx
        bind(vis, sc)
        vis.cull(0, views)

        empty = np.array([((INF,) * 3, 0, (-INF,) * 3, 0)], bs.BOUNDS_DTYPE)

        def good():
            got, _ = check(vis, twin, [0, 1], [basis, basis], boxes, n)
            assert bs.words(got[1:2]) == bs.words(empty)  # a view without draws: the empty answer

        one, twelve = (C.c_uint32 * 9)(*([0] * 9)), (C.c_float * (12 * 9))(*([0.0] * 108))
        out = (GvViewBounds * 8)()
        good()
        assert lib.gv_pool_view_bounds(None, 0, one, twelve, 1) == GV_E_ARG                     # a NULL context
        assert lib.gv_pool_view_bounds(ctx, 5, one, twelve, 1) == GV_E_ARG                      # an unbound pool
        assert lib.gv_pool_view_bounds(ctx, 99, one, twelve, 1) == GV_E_ARG
        assert lib.gv_pool_view_bounds(ctx, 0, one, twelve, 0) == GV_E_ARG                      # item_count 0
        assert lib.gv_pool_view_bounds(ctx, 0, one, twelve, GV_MAX_BOUNDS_ITEMS + 1) == GV_E_ARG
        assert lib.gv_pool_view_bounds(ctx, 0, None, twelve, 1) == GV_E_ARG                     # NULL view_indices
        assert lib.gv_pool_view_bounds(ctx, 0, one, None, 1) == GV_E_ARG                        # NULL bases
        assert code(vis.view_bounds_issue, 0, [GV_MAX_VIEWS], [basis]) == GV_E_ARG              # a view index out of range
        assert code(vis.view_bounds_issue, 0, [0, 6], [basis, basis]) == GV_E_ARG               # not a view of the pool
        good()
        assert lib.gv_pool_view_bounds_fetch(ctx, 0, out, 1) == GV_E_ARG                        # capacity below the item count
        assert lib.gv_pool_view_bounds_fetch(ctx, 0, None, 8) == GV_E_ARG
        assert lib.gv_pool_view_bounds_fetch(None, 0, out, 8) == GV_E_ARG
        assert lib.gv_pool_view_bounds_device(ctx, 0, None, None) == GV_E_ARG
        good()
        assert code(vis.view_bounds_issue, 0, [0, 2], [basis, basis]) == GV_E_STATE             # a count-only view
        good()
        vis.cull(0, views[:2])
        assert code(vis.view_bounds_fetch, 0) == GV_E_STATE                                     # no result since the pool's last cull
        assert code(vis.view_bounds_device, 0) == GV_E_STATE
        assert code(vis.view_bounds_issue, 0, [2], [basis]) == GV_E_STATE                       # a view the last cull ended: no results
        good()
        # a non-finite basis is not an error
        vis.view_bounds(0, [0], [bs.extreme_basis()])
        good()


def test_an_empty_pool_gives_the_empty_answer():
    sc = scene.flat_scene(8, seed=scene.SEED)
    with GpuVisibility(device=0) as vis:
        vis.bind_transforms(sc.transforms, sc.entity_to_transform)
        vis.bind_pool(0, sc.meshes[:0])
        vis.cull(0, [bs.enclosing()])
        got = vis.view_bounds(0, [0, 0], [bs.IDENTITY, bs.rotation_basis(13)])
        for item in got:
            assert item["lo"].tolist() == [np.inf] * 3 and item["hi"].tolist() == [-np.inf] * 3
            assert int(item["draw_count"]) == 0 and int(item["nan_records"]) == 0


# ---- 8. the drop-in's shim -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def view_bounds_driver(tmp_path_factory):
    """tests/cpp/view_bounds.cpp, built by its own tests/cpp/view_bounds.mk"""
    out = str(tmp_path_factory.mktemp("view_bounds"))
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "view_bounds.mk", "OUT=" + out], check=True, timeout=300)
    return os.path.join(out, "view_bounds")


def test_shim_matches_the_host_loop(view_bounds_driver):
    """GpuViewBounds::request / fetch against a host loop over the delivered light-pass list: 20 000 entities with movers, four
    ticks, two bases — all 32 bytes of every item"""
    p = subprocess.run([view_bounds_driver, "--entities", "20000", "--ticks", "4"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = json.loads([line for line in p.stdout.splitlines() if line.startswith("{")][-1])
    assert out["ok"] and out["ticks"] == 4 and out["draws"] > 1000 and "view_bounds ok" in p.stdout, out
