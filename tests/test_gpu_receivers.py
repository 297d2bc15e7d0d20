"""gv_pool_draw_receivers on the device: the cull AABBs of a view's draws rasterised outwards into a receiver mask in a light's clip
space. Expected values come from the C twin of the rule (tests/receiver_twin.h) applied to the records FETCHED in front of the call
and the cull AABBs of their pool slots, and are exact: every word of the mask and all counts. The end-to-end shadow frame is held to
the oracle's cull over the pyramid of the TWIN's mask, to self-keeping, and — against the geometry, not the rule — to rays cast from
the visible receivers towards the light. Sizes and worlds: tests/receivers_support.py, which reads the kernel header."""
import numpy as np
import pytest

import commands_support as csup
import occluders_support as osup
import receivers_support as rs
from garden_amd import scene
from garden_amd.lib import GV_E_ARG, GV_E_STATE, GV_MAX_VIEWS, KERNEL_NAMES, GpuVisibility, GvError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return rs.build_twin(tmp_path_factory.mktemp("receiver_twin"))


def bind(vis, sc, pool_id=0):
    vis.bind_transforms(sc.transforms, sc.entity_to_transform)
    vis.bind_pool(pool_id, sc.meshes)
    vis.hierarchy_rebuild()


def fetch(vis, view, occupancy, pool_id=0, order="raw"):
    return vis.fetch(view, write_back=False, occupancy=occupancy, order=order, pool_id=pool_id)


def code(fn, *args, **kw):
    with pytest.raises(GvError) as e:
        fn(*args, **kw)
    return e.value.code


def draw_and_check(vis, twin, draws, light, width, height):
    """One mask: begin, then for every (pool, view index, cull AABBs by slot, occupancy) of `draws` the records are fetched, the twin
    accumulates them and the device draws them. Every word of the mask and the counts must agree. Returns (mask, counts, the fetched
    results in order)."""
    vis.receiver_begin(width, height)
    image, counts, fetched = None, None, []
    for pool_id, index, boxes, occupancy in draws:
        f = fetch(vis, index, occupancy, pool_id)
        fetched.append(f)
        image, counts = rs.expected(twin, f, boxes, light, width, height, image, counts)
        vis.draw_receivers(pool_id, index, light)
    got_image, got_counts = vis.receiver_mask()
    assert got_image.shape == (height, width)
    print(f"receivers {width}x{height}: device {got_counts}, twin {counts}")
    assert got_counts == counts and got_counts["reserved"] == 0
    difference = osup.first_difference(got_image, image)
    assert difference is None, difference
    return got_image, got_counts, fetched


# ---- 1. bit parity at lane, wave, workgroup and tile edges ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", rs.RECORD_COUNTS)
def test_every_word_and_count_equals_the_twin(n, twin):
    """n records (every slot is a draw of the source view) into every mask size under an orthographic cascade that is not the source
    view's matrix: boxes from sub-pixel to larger than the mask, mirrored, flat, wholly outside; both forms of the setup launch and
    every tile path, asserted on the twin over the device's own records"""
    sc = rs.parity_world(n)
    boxes = rs.aabbs_by_slot(sc.meshes)
    view, light = rs.parity_view(), rs.parity_light()
    assert np.abs(light - view["view_proj"]).max() > 0.01
    seen = dict.fromkeys(rs.FORM_NAMES, 0)
    classes = dict.fromkeys(rs.COUNT_NAMES, 0)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.cull(0, [view])
        for width, height in rs.IMAGE_SIZES:
            image, counts, fetched = draw_and_check(vis, twin, [(0, 0, boxes, n)], light, width, height)
            assert int(fetched[0]["draw_count"]) == n == sum(counts.values())
            assert n < 63 or len(np.unique(rs.words(image))) >= min(width * height, 20)  # (no one box floors the whole mask)
            if width <= 2 * rs.T + 1:  # (the census goes pixel by pixel on the host: the larger masks are left to the parity itself)
                for k, v in rs.forms(twin, fetched[0], boxes, light, width, height).items():
                    seen[k] += v
            for k, v in counts.items():
                classes[k] += v
        if n > 64:
            assert fetched[0]["visible_idx"][:n].tolist() != list(range(n))  # (the mirror's own order is in play)
    if n >= 255:
        assert classes["drawn"] > n and classes["flat"] > 5 and classes["outside"] > 5
        assert seen["small"] > 20 and seen["listed"] > 20 and seen["tiles_all"] > 5 and seen["tiles_some"] > 5 and seen["tiles_none"] > 0, seen


@pytest.mark.parametrize("which", ("inside", "outside"))
def test_a_perspective_light_that_records_reach_behind(which, twin):
    """inside the cloud about half of the records have a corner behind L; from outside a few of the largest do. Either way the whole
    mask is +0.0f, through the item walk as a full-screen box, and the other records are still classed and counted"""
    n = 257
    sc = rs.parity_world(n, seed=3)
    boxes = rs.aabbs_by_slot(sc.meshes)
    view = rs.parity_view()
    light = rs.perspective_light_inside() if which == "inside" else rs.perspective_light_outside()
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.cull(0, [view])
        for width, height in ((2 * rs.T + 1, 2 * rs.T + 1), (100, 40)):
            image, counts, fetched = draw_and_check(vis, twin, [(0, 0, boxes, n)], light, width, height)
            assert counts["behind"] > 0 and counts["drawn"] > 20 and (rs.words(image) == 0).all()
            if which == "outside":
                assert counts["behind"] < n // 4


def test_a_mask_without_a_draw_is_all_infinity_and_a_far_corner_fills_it(twin):
    sc = rs.parity_world(64, seed=1)
    sc.transforms["scale"][7, :3] = (4.0e6, 1.0, 1.0)  # u * 16 W beyond 2^22: `range`
    boxes = rs.aabbs_by_slot(sc.meshes)
    view, light = rs.parity_view(), rs.parity_light()
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.cull(0, [view])
        vis.receiver_begin(40, 30)
        empty, counts = vis.receiver_mask()
        assert (rs.words(empty) == rs.INF_WORD).all() and sum(counts.values()) == 0
        image, counts, _ = draw_and_check(vis, twin, [(0, 0, boxes, 64)], light, 40, 30)
        assert counts["range"] == 1 and np.isfinite(image).all()


@pytest.mark.parametrize("keep_slot_order", (False, True))
def test_both_mirror_orders_sorted_and_grouped_views(keep_slot_order, twin):
    """records are read in delivery order, whatever made it; the mask is the same in every order (the minimum does not care)"""
    n = 3000
    sc = rs.parity_world(n, seed=5)
    boxes = rs.aabbs_by_slot(sc.meshes)
    view, light = rs.parity_view(), rs.parity_light()
    with GpuVisibility(device=0, keep_slot_order=keep_slot_order) as vis:
        bind(vis, sc)
        vis.cull(0, [view])
        image, counts, fetched = draw_and_check(vis, twin, [(0, 0, boxes, n)], light, 96, 80)
        order = fetched[0]["visible_idx"][:n].copy()
        assert (np.diff(order.astype(np.int64)) > 0).all() == keep_slot_order
        vis.sort(0, descending=True, pool_id=0)
        sorted_image, sorted_counts, fetched = draw_and_check(vis, twin, [(0, 0, boxes, n)], light, 96, 80)
        assert fetched[0]["visible_idx"][:n].tolist() != order.tolist()
        ids = np.random.Generator(np.random.PCG64(n)).integers(0, 12, n).astype(np.uint32)
        vis.bind_geometry(0, ids, csup.geometry_table([(3 * (g + 1), 100 * g, g) for g in range(12)]))
        vis.cull(0, [view])
        vis.group_draws(0, pool_id=0)
        grouped_image, grouped_counts, fetched = draw_and_check(vis, twin, [(0, 0, boxes, n)], light, 96, 80)
        assert (np.diff(ids[fetched[0]["visible_idx"][:n]].astype(np.int64)) >= 0).all()
        assert counts == sorted_counts == grouped_counts
        assert rs.words(image).tolist() == rs.words(sorted_image).tolist() == rs.words(grouped_image).tolist()


def test_two_pools_and_two_views_into_one_mask(twin):
    a, b = rs.parity_world(300, seed=1), rs.parity_world(513, seed=2)
    b.meshes["entity"] += 300  # one transform pool for both mesh pools: entity e lives in transform slot e - 1
    transforms = np.concatenate([a.transforms, b.transforms])
    transforms["entity"] = np.arange(1, 814, dtype=np.uint32)
    e2t = np.concatenate([[scene.GV_NONE], np.arange(813)]).astype(np.uint32)
    wide, narrow, light = rs.parity_view(), rs.parity_view(fov=40.0), rs.parity_light()
    with GpuVisibility(device=0) as vis:
        vis.bind_transforms(transforms, e2t)
        vis.bind_pool(0, a.meshes)
        vis.bind_pool(1, b.meshes)
        vis.hierarchy_rebuild()
        vis.cull(0, [wide, narrow])
        vis.cull(1, [wide])
        image, counts, fetched = draw_and_check(vis, twin, [(0, 0, rs.aabbs_by_slot(a.meshes), 300), (1, 0, rs.aabbs_by_slot(b.meshes), 513),
                                                            (0, 1, rs.aabbs_by_slot(a.meshes), 300)], light, 96, 80)
        assert [int(f["draw_count"]) for f in fetched[:2]] == [300, 513] and 0 < int(fetched[2]["draw_count"]) <= 300
        assert sum(counts.values()) == 813 + int(fetched[2]["draw_count"])
        alone, _, _ = draw_and_check(vis, twin, [(1, 0, rs.aabbs_by_slot(b.meshes), 513)], light, 96, 80)
        assert rs.words(alone).tolist() != rs.words(image).tolist()


def test_three_scan_turns(twin):
    """2 * 1024 * 256 + 1 records: the scan between the two launches takes three turns, the last for one block of one record, which
    is listed; nearly all the others are written by the setup launch"""
    n = 2 * 1024 * rs.BLOCK + 1
    sc = rs.parity_world(n)
    large = np.zeros(n, bool)
    large[::509] = True
    large[n - 1] = True
    sc.transforms["scale"][~large, :3] *= np.float32(0.01)
    sc.transforms["scale"][n - 1, :3] = (9.0, 7.0, 5.0)
    boxes = rs.aabbs_by_slot(sc.meshes)
    view, light = rs.parity_view(), rs.parity_light()
    with GpuVisibility(device=0, keep_slot_order=True) as vis:
        bind(vis, sc)
        vis.cull(0, [view])
        image, counts, fetched = draw_and_check(vis, twin, [(0, 0, boxes, n)], light, 96, 80)
    assert int(fetched[0]["draw_count"]) == n == sum(counts.values()) and int(fetched[0]["visible_idx"][n - 1]) == n - 1
    f = rs.forms(twin, fetched[0], boxes, light, 96, 80)
    last = rs.twin_forms(twin, fetched[0]["baked_model"][n - 1:n], boxes[n - 1:n], light, 96, 80)
    assert f["small"] > n // 4 and 500 < f["listed"] < 50_000 and last["listed"] == 1


# ---- 2. end to end: the main view's mask, its pyramid, the cascade's cull against it -------------------------------------------------------

@pytest.fixture(scope="module", params=(False, True), ids=("rg32f", "rg16f"))
def shadow_frame(request, twin):
    """the frame on the device, once per pyramid format: dict(e: the oracle's side, main, plain, masked: the device's fetched results in
    slot order, image, counts)"""
    rg16f = request.param
    e = rs.shadow_oracle(rg16f)
    sc, slots = rs.shadow_world()
    n = sc.count
    boxes = rs.aabbs_by_slot(sc.meshes)
    main_view, light, plain_view, masked_view = rs.shadow_views()
    width, height = rs.SHADOW_MASK
    with GpuVisibility(device=0, hiz_rg16f=rg16f) as vis:
        bind(vis, sc)
        vis.cull(0, [main_view, plain_view])
        plain = fetch(vis, 1, n, order="slot")
        image, counts, fetched = draw_and_check(vis, twin, [(0, 0, boxes, n)], light, width, height)
        main = fetch(vis, 0, n, order="slot")
        vis.hiz_build_from_receivers()
        assert code(vis.draw_receivers, 0, 0, light) == GV_E_STATE  # (the build closed the mask)
        vis.cull(0, [masked_view])
        masked = fetch(vis, 0, n, order="slot")
    return dict(e=e, sc=sc, slots=slots, boxes=boxes, light=light, main=main, plain=plain, masked=masked, image=image, counts=counts)


def slots_of(fetched):
    return np.asarray(fetched["visible_idx"])[:int(fetched["draw_count"])].astype(np.int64)


def test_the_masked_cascade_equals_the_oracles_cull_over_the_pyramid_of_the_twins_mask(shadow_frame):
    f, e = shadow_frame, shadow_frame["e"]
    assert rs.words(f["image"]).tolist() == rs.words(e["image"]).tolist() and f["counts"] == e["counts"]
    for name in ("main", "plain", "masked"):
        got, want = f[name], e[name]
        assert int(got["draw_count"]) == int(want["draw_count"]), name
        assert slots_of(got).tolist() == np.asarray(want["visible_idx"]).tolist(), name
        assert got["baked_model"].view(np.uint32).tolist() == np.asarray(want["baked_model"], np.float32).view(np.uint32).tolist(), name
    assert int(f["masked"]["draw_count"]) <= int(f["plain"]["draw_count"]) - 100


def test_what_the_main_view_sees_keeps_itself_in_the_cascade(shadow_frame):
    f = shadow_frame
    main, plain, masked = (set(slots_of(f[k]).tolist()) for k in ("main", "plain", "masked"))
    assert masked <= plain and len(main & plain) >= 1000
    assert (main & plain) <= masked


def test_by_hand_under_the_floor_over_nothing_and_over_the_floor(shadow_frame):
    f, slots = shadow_frame, shadow_frame["slots"]
    main, plain, masked = (set(slots_of(f[k]).tolist()) for k in ("main", "plain", "masked"))
    assert slots["floor"] in main and slots["floor"] in masked
    width, height = rs.SHADOW_MASK
    for name, slot in slots.items():
        if name == "floor":
            continue
        assert slot not in main and slot in plain, name
        assert (slot in masked) == name.startswith("above_floor"), name
    order = slots_of(f["plain"]).tolist()
    models = np.asarray(f["plain"]["baked_model"], np.float32).reshape(-1, 12)
    for name in ("off_floor_0", "off_floor_1"):
        s = rs.twin_setup(rs.shared_twin(), models[order.index(slots[name])], f["boxes"][slots[name]], f["light"], width, height)
        x0, x1, y0, y1 = s["range"]
        assert x0 >= 8 and y0 >= 8 and x1 + 8 < width and y1 + 8 < height
        assert (rs.words(f["image"][y0 - 8:y1 + 9, x0 - 8:x1 + 9]) == rs.INF_WORD).all(), name


def test_no_ray_from_a_visible_receiver_towards_the_light_hits_a_dropped_caster(shadow_frame):
    """against the geometry, not the rule: 4 096 points inside the cull AABBs of what the device's main view delivered, at least two
    texels inside the mask, cast towards the light and slab-tested against every caster the device's frustum-only cascade cull kept
    and its masked cull dropped"""
    f = shadow_frame
    width, height = rs.SHADOW_MASK
    plain, masked = slots_of(f["plain"]), set(slots_of(f["masked"]).tolist())
    models = np.asarray(f["plain"]["baked_model"], np.float32).reshape(-1, 12)
    dropped = [k for k, s in enumerate(plain.tolist()) if s not in masked]
    kept = [k for k, s in enumerate(plain.tolist()) if s in masked and s != f["slots"]["floor"]][:2000]
    assert len(dropped) >= 100
    points = rs.sample_points(f["main"], f["boxes"], f["light"], width, height, floor_slot=f["slots"]["floor"])
    assert len(points) == 4096
    towards_light = -np.asarray(rs.LIGHT_DIR, np.float64) / np.linalg.norm(rs.LIGHT_DIR)
    hits_dropped = rs.rays_hit(points, towards_light, models[dropped], f["boxes"][plain[dropped]], f["light"])
    hits_kept = rs.rays_hit(points, towards_light, models[kept], f["boxes"][plain[kept]], f["light"])
    print(f"rays: {int(hits_dropped.sum())} hit a dropped caster, {int(hits_kept.sum())} a kept one; {len(dropped)} casters dropped")
    assert not hits_dropped.any(), int(hits_dropped.sum())
    assert hits_kept.sum() >= 100


# ---- 3. lifetimes and errors ---------------------------------------------------------------------------------------------------------------

def test_the_pyramids_mask_is_never_redrawn_and_an_occluder_image_may_be_open_alongside(twin):
    n = 300
    sc = rs.parity_world(n, seed=7)
    boxes = rs.aabbs_by_slot(sc.meshes)
    lo, hi = osup.occluder_boxes(sc.meshes, seed=7)
    view, light = rs.parity_view(), rs.parity_light()
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_occluders(0, lo, hi)
        vis.cull(0, [view])
        vis.occluder_begin(48, 32)
        vis.draw_occluders(0, 0, 1)
        first, _, _ = draw_and_check(vis, twin, [(0, 0, boxes, n)], light, 64, 48)
        occluders, _ = vis.occluder_depth()  # (the draw into the mask left the open occluder image alone, and it is still open)
        vis.draw_occluders(0, 0, 1)
        vis.hiz_build_from_receivers()
        pointer = vis.receiver_mask_device()[0]
        levels = [vis.hiz_read_level(k, max(64 >> k, 1), max(48 >> k, 1)).view(np.uint32).copy() for k in range(1, vis.hiz_mip_count())]
        vis.receiver_begin(37, 23)  # takes the other image
        assert vis.receiver_mask_device()[0] != pointer
        vis.draw_receivers(0, 0, light)
        other, _ = vis.receiver_mask()
        assert other.shape == (23, 37) and np.isfinite(other).any()
        vis.receiver_begin(64, 48)  # (starting over keeps away from the pyramid's image too)
        assert vis.receiver_mask_device()[0] != pointer
        vis.hiz_rebuild()
        again = [vis.hiz_read_level(k, max(64 >> k, 1), max(48 >> k, 1)).view(np.uint32).copy() for k in range(1, vis.hiz_mip_count())]
        assert all(a.tolist() == b.tolist() for a, b in zip(again, levels))
        assert rs.words(vis.occluder_depth()[0]).tolist() == rs.words(occluders).tolist()
        vis.hiz_build_from_occluders()  # the pyramid moves to the occluder image: both receiver images are free again
        vis.receiver_begin(64, 48)
        again_first, _, _ = draw_and_check(vis, twin, [(0, 0, boxes, n)], light, 64, 48)
        assert rs.words(again_first).tolist() == rs.words(first).tolist()


def test_argument_and_state_errors():
    n = 64
    sc = rs.parity_world(n)
    view, light = rs.parity_view(), rs.parity_light()
    with GpuVisibility(device=0) as vis:
        assert code(vis.receiver_mask_device) == GV_E_STATE  # no begin yet
        assert code(vis.hiz_build_from_receivers) == GV_E_STATE
        assert code(vis.receiver_begin, 0, 8) == GV_E_ARG and code(vis.receiver_begin, 8, 32769) == GV_E_ARG
        assert code(vis.draw_receivers, 0, 0, light) == GV_E_ARG  # the pool is not bound
        bind(vis, sc)
        assert vis.lib.gv_pool_draw_receivers(vis.ctx, 0, 0, None) == GV_E_ARG
        assert code(vis.draw_receivers, 0, GV_MAX_VIEWS, light) == GV_E_ARG
        assert code(vis.draw_receivers, 0, 0, light) == GV_E_ARG  # never a view of the pool
        vis.cull(0, [view, rs.parity_view(emit_records=0), view])
        assert code(vis.draw_receivers, 0, 0, light) == GV_E_STATE  # no open mask
        vis.receiver_begin(16, 16)
        assert code(vis.draw_receivers, 0, 1, light) == GV_E_STATE  # count-only
        vis.cull(0, [view])
        assert code(vis.draw_receivers, 0, 2, light) == GV_E_STATE  # a later cull of fewer views ended it
        vis.draw_receivers(0, 0, light)
        image = np.zeros((16, 16), np.float32)
        assert vis.lib.gv_receiver_mask_fetch(vis.ctx, image.ctypes.data, image.nbytes - 1, None) == GV_E_ARG
        assert vis.lib.gv_receiver_mask_fetch(vis.ctx, None, 0, None) == GV_E_ARG
        _, counts = vis.receiver_mask()
        assert sum(counts.values()) == n
        launches = vis.stats()["launches"]
        vis.draw_receivers(0, 0, light)
        after = vis.stats()["launches"]
        assert sum(after.values()) - sum(launches.values()) == 3  # three launches whatever the counts, all under GV_K_HIZ
        assert after[KERNEL_NAMES[3]] - launches[KERNEL_NAMES[3]] == 3
