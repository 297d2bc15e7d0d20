"""gv_pool_draw_occluders on the device: the occluder boxes of a view's draws rasterised into a depth image. Expected values come from
the C twin of the rule (tests/occluder_twin.h) applied to the records FETCHED in front of the call and the occluder boxes of their
pool slots, and are exact: every word of the image and all six counts. The record counts, image sizes and the tile size come from
tests/occluders_support.py, which reads the kernel header; the end-to-end frame is held to the oracle's cull over the TWIN's image."""
import numpy as np
import pytest

import commands_support as csup
import occluders_support as osup
import second_phase_support as sp
from garden_amd import scene
from garden_amd.lib import GV_DIRTY_OCCLUDER, GV_E_ARG, GV_E_STATE, GV_MAX_VIEWS, GpuVisibility, GvError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return osup.build_twin(tmp_path_factory.mktemp("occluder_twin"))


def bind(vis, sc, lo=None, hi=None, pool_id=0):
    vis.bind_transforms(sc.transforms, sc.entity_to_transform)
    vis.bind_pool(pool_id, sc.meshes)
    vis.hierarchy_rebuild()
    if lo is not None:
        vis.bind_occluders(pool_id, lo, hi)


def fetch(vis, view, occupancy, pool_id=0, order="raw"):
    return vis.fetch(view, write_back=False, occupancy=occupancy, order=order, pool_id=pool_id)


def code(fn, *args, **kw):
    with pytest.raises(GvError) as e:
        fn(*args, **kw)
    return e.value.code


def draw_and_check(vis, twin, draws, width, height, min_pixels=1):
    """One image: begin, then for every (pool, view index, view, boxes by slot, occupancy) of `draws` the records are fetched, the twin
    accumulates them and the device draws them. Every word of the image and the six counts must agree. Returns (image, counts, the
    fetched results in order)."""
    vis.occluder_begin(width, height)
    image, counts, fetched = None, None, []
    for pool_id, index, view, boxes, occupancy in draws:
        f = fetch(vis, index, occupancy, pool_id)
        fetched.append(f)
        image, counts = osup.expected(twin, f, boxes, view["view_proj"], width, height, min_pixels, image, counts)
        vis.draw_occluders(pool_id, index, min_pixels)
    got_image, got_counts = vis.occluder_depth()
    assert got_image.shape == (height, width)
    assert got_counts == counts
    assert osup.words(got_image).tolist() == osup.words(image).tolist()
    return got_image, got_counts, fetched


# ---- 1. bit parity at lane, wave, workgroup and tile edges ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", osup.RECORD_COUNTS)
def test_every_word_and_count_equals_the_twin(n, twin):
    """n records (every slot is a draw) into every image size; boxes from sub-pixel to larger than the screen, mirrored ones, some
    that reach behind the camera, slots without a box"""
    sc = osup.parity_world(n)
    lo, hi = osup.occluder_boxes(sc.meshes)
    boxes = osup.boxes_by_slot(lo, hi)
    view = osup.parity_view()
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, lo, hi)
        vis.cull(0, [view])
        written = 0
        for width, height in osup.IMAGE_SIZES:
            image, counts, fetched = draw_and_check(vis, twin, [(0, 0, view, boxes, n)], width, height)
            assert int(fetched[0]["draw_count"]) == n == sum(counts.values())
            written += int(np.count_nonzero(image))
        if n >= 63:
            assert counts["drawn"] > n // 4 and counts["no_box"] > 0 and written > 1000
        if n > 64:
            assert fetched[0]["visible_idx"][:n].tolist() != list(range(n))  # (the mirror's own order is in play)


def test_a_full_screen_occluder_takes_all_three_tile_paths(twin):
    """(2 T + 1)^2: the plate holds the first tile whole, cuts the second, and the corner pixel's tile lies outside an edge — asserted
    on the twin over the device's own record"""
    side = 2 * osup.T + 1
    sc = scene.flat_scene(1, seed=scene.SEED + 0x0CC7, defects=False)
    sc.transforms["position"][0, :3] = (-0.6, 0.6, 3.0)
    sc.transforms["scale"][0, :3] = (3.6, 3.6, 0.05)
    sc.transforms["rotation"][0] = (0.0, 0.0, 0.38268343, 0.92387953)
    sc.meshes["aabbMin"][0, :3], sc.meshes["aabbMax"][0, :3] = -1.0, 1.0
    lo, hi = sc.meshes["aabbMin"].copy(), sc.meshes["aabbMax"].copy()
    view = scene.make_view(osup.camera(1.0))
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, lo, hi)
        vis.cull(0, [view])
        image, counts, fetched = draw_and_check(vis, twin, [(0, 0, view, osup.boxes_by_slot(lo, hi), 1)], side, side)
        assert counts["drawn"] == 1
        inside, mixed, outside = osup.twin_paths(twin, fetched[0]["baked_model"][:1], osup.boxes_by_slot(lo, hi)[:1], view["view_proj"], side, side)
        assert inside >= 1 and mixed >= 1 and outside >= 1
        assert osup.T * osup.T < np.count_nonzero(image) < side * side


@pytest.mark.parametrize("keep_slot_order", (False, True))
def test_both_mirror_orders_sorted_and_grouped_views(keep_slot_order, twin):
    """records are read in delivery order, whatever made it; the image is the same in every order (the maximum does not care)"""
    n = 3000
    sc = osup.parity_world(n, seed=5)
    lo, hi = osup.occluder_boxes(sc.meshes, seed=5)
    boxes = osup.boxes_by_slot(lo, hi)
    view = osup.parity_view()
    with GpuVisibility(device=0, keep_slot_order=keep_slot_order) as vis:
        bind(vis, sc, lo, hi)
        vis.cull(0, [view])
        image, counts, fetched = draw_and_check(vis, twin, [(0, 0, view, boxes, n)], 64, 48)
        order = fetched[0]["visible_idx"][:n].copy()
        assert (np.diff(order.astype(np.int64)) > 0).all() == keep_slot_order
        vis.sort(0, descending=True, pool_id=0)
        sorted_image, sorted_counts, fetched = draw_and_check(vis, twin, [(0, 0, view, boxes, n)], 64, 48)
        assert fetched[0]["visible_idx"][:n].tolist() != order.tolist()
        ids = np.random.Generator(np.random.PCG64(n)).integers(0, 12, n).astype(np.uint32)
        vis.bind_geometry(0, ids, csup.geometry_table([(3 * (g + 1), 100 * g, g) for g in range(12)]))
        vis.cull(0, [view])
        vis.group_draws(0, pool_id=0)
        grouped_image, grouped_counts, fetched = draw_and_check(vis, twin, [(0, 0, view, boxes, n)], 64, 48)
        assert (np.diff(ids[fetched[0]["visible_idx"][:n]].astype(np.int64)) >= 0).all()
        assert counts == sorted_counts == grouped_counts
        assert osup.words(image).tolist() == osup.words(sorted_image).tolist() == osup.words(grouped_image).tolist()


def test_two_pools_and_two_views_into_one_image(twin):
    a, b = osup.parity_world(300, seed=1), osup.parity_world(513, seed=2)
    b.meshes["entity"] += 300  # one transform pool for both mesh pools: entity e lives in transform slot e - 1
    transforms = np.concatenate([a.transforms, b.transforms])
    transforms["entity"] = np.arange(1, 814, dtype=np.uint32)
    e2t = np.concatenate([[scene.GV_NONE], np.arange(813)]).astype(np.uint32)
    lo_a, hi_a = osup.occluder_boxes(a.meshes, seed=1)
    lo_b, hi_b = osup.occluder_boxes(b.meshes, seed=2)
    wide, narrow = osup.parity_view(), osup.parity_view(fov=40.0)
    with GpuVisibility(device=0) as vis:
        vis.bind_transforms(transforms, e2t)
        vis.bind_pool(0, a.meshes)
        vis.bind_pool(1, b.meshes)
        vis.hierarchy_rebuild()
        vis.bind_occluders(0, lo_a, hi_a)
        vis.bind_occluders(1, lo_b, hi_b)
        vis.cull(0, [wide, narrow])
        vis.cull(1, [wide])
        image, counts, fetched = draw_and_check(vis, twin, [(0, 0, wide, osup.boxes_by_slot(lo_a, hi_a), 300),
                                                            (1, 0, wide, osup.boxes_by_slot(lo_b, hi_b), 513),
                                                            (0, 1, narrow, osup.boxes_by_slot(lo_a, hi_a), 300)], 64, 48)
        assert [int(f["draw_count"]) for f in fetched[:2]] == [300, 513] and 0 < int(fetched[2]["draw_count"]) <= 300
        assert sum(counts.values()) == 813 + int(fetched[2]["draw_count"])
        alone, _, _ = draw_and_check(vis, twin, [(1, 0, wide, osup.boxes_by_slot(lo_b, hi_b), 513)], 64, 48)
        assert osup.words(alone).tolist() != osup.words(image).tolist()


# ---- 2. every skip class, on the device -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_pixels", (1, 8))
def test_every_skip_class_is_hit(min_pixels, twin):
    sc, lo, hi, names = osup.skip_world()
    view = scene.make_view(osup.camera(1.0))
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, lo, hi)
        vis.cull(0, [view])
        image, counts, fetched = draw_and_check(vis, twin, [(0, 0, view, osup.boxes_by_slot(lo, hi), len(names))], 64, 64, min_pixels)
        assert int(fetched[0]["draw_count"]) == len(names)
        small = int(min_pixels == 8)  # (the sub-pixel box has a range of one pixel: drawn, covering nothing, at min_pixels = 1)
        assert counts == dict(drawn=2 - small, no_box=2, behind=1, range=1, flat=1, small=small)
        assert np.count_nonzero(image) == 18 * 8  # the one box that covers pixels: tests/test_occluder_twin.py works its rectangle out


# ---- 3. marks ----------------------------------------------------------------------------------------------------------------------------

def test_a_marked_edit_changes_the_next_image_and_an_unmarked_one_does_not(twin):
    n = 700
    sc = osup.parity_world(n, seed=9)
    lo, hi = osup.occluder_boxes(sc.meshes, seed=9)
    view = osup.parity_view()
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, lo, hi)
        vis.cull(0, [view])
        before, counts, fetched = draw_and_check(vis, twin, [(0, 0, view, osup.boxes_by_slot(lo, hi), n)], 64, 48)
        uploaded = vis.stats()["upload_bytes"]
        # a slot whose box the image depends on loses it; nobody is told
        held = osup.boxes_by_slot(lo, hi)
        slot = None
        for candidate in fetched[0]["visible_idx"][:n]:
            without = held.copy()
            without[candidate] = 0.0
            if osup.words(osup.expected(twin, fetched[0], without, view["view_proj"], 64, 48)[0]).tolist() != osup.words(before).tolist():
                slot = int(candidate)
                break
        assert slot is not None
        kept = hi[slot].copy()
        hi[slot] = lo[slot]
        unmarked, _, _ = draw_and_check(vis, twin, [(0, 0, view, held, n)], 64, 48)  # (expected: the boxes as they were)
        assert osup.words(unmarked).tolist() == osup.words(before).tolist() and vis.stats()["upload_bytes"] == uploaded
        vis.mark_dirty(GV_DIRTY_OCCLUDER, slot, 1, pool_id=0)
        marked, marked_counts, _ = draw_and_check(vis, twin, [(0, 0, view, osup.boxes_by_slot(lo, hi), n)], 64, 48)
        assert osup.words(marked).tolist() != osup.words(before).tolist() and marked_counts["no_box"] == counts["no_box"] + 1
        assert 0 < vis.stats()["upload_bytes"] - uploaded <= 64  # one 32-byte row and its slot word
        hi[slot] = kept
        vis.mark_dirty(GV_DIRTY_OCCLUDER, slot, 1, pool_id=0)
        again, _, _ = draw_and_check(vis, twin, [(0, 0, view, osup.boxes_by_slot(lo, hi), n)], 64, 48)
        assert osup.words(again).tolist() == osup.words(before).tolist()


# ---- 4. end to end: cull, draw, build, cull against the new pyramid ---------------------------------------------------------------------

def pyramid(vis, width, height):
    levels = []
    for level in range(1, vis.hiz_mip_count()):
        levels.append(vis.hiz_read_level(level, max(width >> level, 1), max(height >> level, 1)).view(np.uint32).copy())
    return levels


def test_a_headless_frame_culls_what_the_walls_hide(twin):
    width, height = 64, 48
    sc, lo, hi = osup.wall_world()
    n = sc.count
    e = osup.oracle_cull()
    frustum, full = e["first"], e["full"]
    # the scene is worth the test: the walls hide entities the frustum keeps, and the nearest wall is hidden by nothing
    assert int(full["draw_count"]) < int(frustum["draw_count"]) - 20 and 0 in full["visible_idx"] and e["counts"]["drawn"] == osup.WALLS
    plain, hiz_view, zoomed = osup.parity_view(), osup.parity_view(use_hiz=1), osup.parity_view(fov=50.0)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, lo, hi)
        vis.cull(0, [plain])
        image, counts, _ = draw_and_check(vis, twin, [(0, 0, plain, osup.boxes_by_slot(lo, hi), n)], width, height)
        assert osup.words(image).tolist() == osup.words(e["image"]).tolist() and counts == e["counts"]
        vis.hiz_build_from_occluders()
        assert code(vis.draw_occluders, 0, 0) == GV_E_STATE  # (the build closed the image)
        vis.cull(0, [hiz_view])
        got = fetch(vis, 0, n, order="slot")
        assert int(got["draw_count"]) == int(full["draw_count"])
        assert got["visible_idx"].tolist() == np.asarray(full["visible_idx"]).tolist()
        assert got["baked_model"].view(np.uint32).tolist() == np.asarray(full["baked_model"], np.float32).view(np.uint32).tolist()
        # ... and as a second phase behind a first view that saw only the middle of the screen
        first = sp.oracle_cull(sc, zoomed)
        want = sp.second_of(first, full, n)
        assert 0 < int(want["draw_count"]) < int(full["draw_count"])
        vis.cull(0, [zoomed])
        vis.cull_second_phase(0, 1, hiz_view, pool_id=0)
        second = fetch(vis, 1, n, order="slot")
        assert second["visible_idx"].tolist() == np.asarray(want["visible_idx"]).tolist()
        assert second["baked_model"].view(np.uint32).tolist() == np.asarray(want["baked_model"], np.float32).view(np.uint32).tolist()
        # the pyramid's image is never cleared or redrawn under it: a new begin (another size, other contents) takes the other image
        levels = pyramid(vis, width, height)
        vis.occluder_begin(37, 23)
        vis.draw_occluders(0, 0, 1)
        other, _ = vis.occluder_depth()
        assert other.shape == (23, 37) and other.any()
        vis.occluder_begin(width, height)  # (starting over keeps away from the pyramid's image too)
        vis.hiz_rebuild()
        again = pyramid(vis, width, height)
        assert len(again) == len(levels) and all(a.tolist() == b.tolist() for a, b in zip(again, levels))
        vis.cull(0, [hiz_view])
        assert fetch(vis, 0, n, order="slot")["visible_idx"].tolist() == np.asarray(full["visible_idx"]).tolist()


@pytest.mark.parametrize("seed", range(6))
def test_a_box_equal_to_its_aabb_does_not_hide_its_own_slot(seed, twin):
    """one entity whose occluder box IS its AABB: the query of the same box gets the drawn words back (zNear >= d), so the slot stays
    visible against the pyramid of its own occluder — and the frame equals the oracle's over the twin's image"""
    from oracle import oracle_py
    sc = osup.parity_world(1, seed=40 + seed)
    sc.transforms["scale"][0, :3] = np.float32(12.0) + 10 * seed  # from a few pixels to most of the screen
    lo, hi = sc.meshes["aabbMin"].copy(), sc.meshes["aabbMax"].copy()
    view, hiz_view = osup.parity_view(), osup.parity_view(use_hiz=1)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, lo, hi)
        vis.cull(0, [view])
        image, counts, fetched = draw_and_check(vis, twin, [(0, 0, view, osup.boxes_by_slot(lo, hi), 1)], 64, 48)
        assert counts["drawn"] == 1 and image.any()
        vis.hiz_build_from_occluders()
        vis.cull(0, [hiz_view])
        got = fetch(vis, 0, 1, order="slot")
        want = oracle_py.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, hiz_view, hiz=oracle_py.Hiz(image))
        assert int(got["draw_count"]) == int(want["draw_count"]) == 1


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------------

def test_argument_and_state_errors():
    n = 64
    sc = osup.parity_world(n)
    lo, hi = osup.occluder_boxes(sc.meshes)
    view = osup.parity_view()
    with GpuVisibility(device=0) as vis:
        assert code(vis.occluder_depth_device) == GV_E_STATE  # no begin yet
        assert code(vis.hiz_build_from_occluders) == GV_E_STATE
        assert code(vis.occluder_begin, 0, 8) == GV_E_ARG and code(vis.occluder_begin, 8, 32769) == GV_E_ARG
        assert code(vis.draw_occluders, 0, 0) == GV_E_ARG  # the pool is not bound
        bind(vis, sc)
        assert code(vis.draw_occluders, 0, GV_MAX_VIEWS) == GV_E_ARG
        assert code(vis.draw_occluders, 0, 0) == GV_E_ARG  # never a view of the pool
        vis.cull(0, [view, osup.parity_view(emit_records=0), view])
        assert code(vis.draw_occluders, 0, 0) == GV_E_STATE  # no open image
        vis.occluder_begin(16, 16)
        assert code(vis.draw_occluders, 0, 0) == GV_E_STATE  # no occluder binding
        assert vis.lib.gv_pool_bind_occluders(vis.ctx, 0, lo.ctypes.data, None, 16, n) == GV_E_ARG
        assert vis.lib.gv_pool_bind_occluders(vis.ctx, 0, lo.ctypes.data, hi.ctypes.data, 8, n) == GV_E_ARG
        assert vis.lib.gv_pool_bind_occluders(vis.ctx, 16, lo.ctypes.data, hi.ctypes.data, 16, n) == GV_E_ARG
        vis.bind_occluders(0, lo[:n - 1], hi[:n - 1])
        assert code(vis.draw_occluders, 0, 0) == GV_E_STATE  # boxes below the view's occupancy
        vis.bind_occluders(0, lo, hi)
        assert code(vis.draw_occluders, 0, 1) == GV_E_STATE  # count-only
        vis.cull(0, [view])
        assert code(vis.draw_occluders, 0, 2) == GV_E_STATE  # a later cull of fewer views ended it
        vis.draw_occluders(0, 0)
        image = np.zeros((16, 16), np.float32)
        assert vis.lib.gv_occluder_depth_fetch(vis.ctx, image.ctypes.data, image.nbytes - 1, None) == GV_E_ARG
        assert vis.lib.gv_occluder_depth_fetch(vis.ctx, None, 0, None) == GV_E_ARG
        vis.bind_occluders(0, None, None)
        assert code(vis.draw_occluders, 0, 0) == GV_E_STATE
        _, counts = vis.occluder_depth()
        assert sum(counts.values()) == n
