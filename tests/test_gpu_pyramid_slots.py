"""Pyramid slots on the device: gv_hiz_select / gv_hiz_drop, a view that names its pyramid (GvView::use_hiz = 1 + k), and the batched
pass that holds every view against its own pyramid in ONE cull launch (cull_multi_hiz_kernel). Expected values are the oracle's,
unchanged and exact: prepare_meshes(view, hiz=Hiz(image of the pyramid the view names)). The cases, their images and the census that
keeps them meaningful: tests/pyramid_slots_support.py, tests/test_pyramid_slots_abi.py."""
import functools

import numpy as np
import pytest

import cull_paths_support as cp
import pyramid_slots_support as ps
import receivers_support as rs
from garden_amd import scene
from garden_amd.lib import GV_E_ARG, GV_E_STATE, GV_MAX_PYRAMIDS, GpuVisibility, GvError

pytestmark = pytest.mark.gpu

COUNTED = ("cull", "scan", "emit", "sweep")


@pytest.fixture(scope="module")
def rg16f():
    """a context of this module's own: the pyramids in the reference's RG16F format, the mirror in pool-slot order"""
    vis = GpuVisibility(device=0, hiz_rg16f=True, keep_slot_order=True)
    yield vis
    vis.close()


def code(fn, *args, **kw):
    with pytest.raises(GvError) as e:
        fn(*args, **kw)
    return e.value.code


def bind(vis, sc, pool_id=0):
    vis.bind_transforms(sc.transforms, sc.entity_to_transform)
    vis.bind_pool(pool_id, sc.meshes)
    vis.hierarchy_rebuild()


def private_copy(sc):
    return scene.Scene(sc.meshes.copy(), sc.transforms.copy(), sc.entity_to_transform)


def levels_of(vis, size):
    """every stored level of the selected pyramid as uint32 words"""
    w, h = size
    return [vis.hiz_read_level(k, max(w >> k, 1), max(h >> k, 1)).view(np.uint32).copy() for k in range(1, vis.hiz_mip_count())]


def same_levels(a, b):
    return len(a) == len(b) and all(x.tolist() == y.tolist() for x, y in zip(a, b))


def device_words(vis, pointer, count):
    """`count` 32-bit words at a device pointer, copied to the host behind a wait for the context's stream — through the HIP runtime
    this process has loaded already (found in its own mappings: a second runtime would see no device)"""
    import ctypes
    vis.wait()
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64.so" in line}
    assert len(paths) == 1, paths
    hip = ctypes.CDLL(paths.pop())
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.empty(count, np.uint32)
    assert hip.hipMemcpy(out.ctypes.data, pointer, out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


def back_to_one_pyramid(vis):
    """the session's contexts go on to other tests: pyramid 0 selected, the other slots empty"""
    for k in range(1, GV_MAX_PYRAMIDS):
        vis.hiz_drop(k)
    vis.hiz_select(0)


# ---- 1. every case, every view set, batched and un-batched, against the oracle ------------------------------------------------------------

@pytest.mark.parametrize("c", ps.CASES, ids=lambda c: c.name)
def test_every_view_against_its_own_pyramid(request, oracle, c):
    vis = request.getfixturevalue(c.fixture)
    is_rg16f = c.fixture == "rg16f"
    sc = private_copy(ps.build_scene(c))
    e2t = sc.entity_to_transform
    pyramids = {k: ps.oracle_pyramid(oracle, c, k, is_rg16f) for k in ps.pyramids_of(c)}
    try:
        bind(vis, sc)
        assert vis.stats()["max_depth"] == c.depth
        for k in reversed(ps.pyramids_of(c)):  # (built in descending order: nothing hangs on slot 0 coming first)
            vis.hiz_select(k)
            vis.hiz_build(ps.depth_image(c, k))
            assert vis.hiz_mip_count() == pyramids[k].mip_count
        # the selection between build and cull changes no result: a view names its pyramid itself
        vis.hiz_select((ps.pyramids_of(c)[-1] + 3) % GV_MAX_PYRAMIDS)
        for s in c.sets:
            for shared in (True, False):
                views = ps.make_views(c, s, shared)
                what = f"{c.name} {s} {'batched' if shared else 'one launch per view'}"
                vis.stats_reset()
                vis.cull(0, views)
                launches = vis.stats()["launches"]
                if shared:
                    assert ps.takes_new_form(s) and launches["cull"] == 1, (what, launches)
                else:
                    assert launches["cull"] >= len(views), (what, launches)
                for i, view in enumerate(views):
                    hz = pyramids[ps.pyramid_of(view["use_hiz"])] if view["use_hiz"] else None
                    exp = ps.compare_view(vis, oracle, sc.meshes, sc.transforms, e2t, view, i, hz, f"{what} view {i}")
                    assert c.n < 257 or not view["use_hiz"] or exp["draw_count"] > 0, what
    finally:
        back_to_one_pyramid(vis)


def test_views_that_say_0_or_1_take_the_launches_they_always_took(gpu, oracle):
    """the plan of tests/cull_paths_support.py for a main pass with Hi-Z and a cascade at its position: one batched cull, one batched
    emit — with other pyramids built in other slots and another slot selected"""
    n = 333
    sc = private_copy(cp.build_scene("flat", n, n))
    side = cp.scene_side(n)
    image = scene.synthetic_depth(256, 256)
    try:
        bind(gpu, sc)
        gpu.hiz_build(image)
        gpu.hiz_select(3)
        gpu.hiz_build(scene.synthetic_depth(250, 130, seed=5))
        for codes in ("Eh,Es", "Eh,Es,Es,Es", "E,Es", "Eh,Cs"):
            views = cp.make_views(codes, 3, side)
            plan = cp.cull_plan(n, n, "exact", 0, cp.parse_views(codes), cp.FIXTURE_FLAGS["gpu"])
            gpu.stats_reset()
            gpu.cull(0, views)
            stats = gpu.stats()
            assert {k: stats["launches"][k] for k in COUNTED} == plan.launches, (codes, stats["launches"], plan.launches)
            for i, view in enumerate(views):
                ps.compare_view(gpu, oracle, sc.meshes, sc.transforms, sc.entity_to_transform, view, i, oracle.Hiz(image), f"{codes} view {i}")
    finally:
        back_to_one_pyramid(gpu)


# ---- 2. state --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def state_world():
    sc = cp.build_scene("flat", 4097, 4097)
    c = ps.case("state", "gpu", "flat", 4097, ("1-2", "3-0-1"))
    return sc, c


def test_build_and_rebuild_touch_the_selected_slot_only(state_world):
    sc, c = state_world
    with GpuVisibility(device=0) as vis:
        vis.hiz_build(ps.depth_image(c, 0))
        size0 = ps.image_size(c, 0)
        slot0 = levels_of(vis, size0)
        vis.hiz_select(2)
        assert code(vis.hiz_mip_count) == GV_E_STATE and code(vis.hiz_rebuild) == GV_E_STATE  # slot 2 is not built
        own = ps.depth_image(c, 2).copy()
        vis.hiz_build(own)
        slot2 = levels_of(vis, ps.image_size(c, 2))
        vis.hiz_select(0)
        assert same_levels(levels_of(vis, size0), slot0)  # a build into slot 2 left every byte of slot 0
        vis.hiz_select(2)
        vis.hiz_rebuild()
        assert same_levels(levels_of(vis, ps.image_size(c, 2)), slot2)
        vis.hiz_select(0)
        vis.hiz_rebuild()
        assert same_levels(levels_of(vis, size0), slot0)
        vis.hiz_select(2)
        assert same_levels(levels_of(vis, ps.image_size(c, 2)), slot2)  # ... and a rebuild of slot 0 left slot 2
        # errors: nothing changes
        assert code(vis.hiz_select, GV_MAX_PYRAMIDS) == GV_E_ARG and code(vis.hiz_drop, GV_MAX_PYRAMIDS) == GV_E_ARG
        assert same_levels(levels_of(vis, ps.image_size(c, 2)), slot2)
        vis.hiz_drop(5)  # never built: GV_OK
        vis.hiz_drop(2)  # the selected one
        assert code(vis.hiz_mip_count) == GV_E_STATE
        vis.hiz_select(0)
        assert same_levels(levels_of(vis, size0), slot0)
        vis.hiz_select(1)
        vis.hiz_drop(0)  # a parked one
        vis.hiz_select(0)
        assert code(vis.hiz_mip_count) == GV_E_STATE


def test_a_view_that_names_a_pyramid_nobody_built_is_refused_and_the_results_stay(state_world, oracle):
    sc, c = state_world
    sc = private_copy(sc)
    views = ps.make_views(c, "1-2")
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.hiz_build(ps.depth_image(c, 0))
        hz0 = ps.oracle_pyramid(oracle, c, 0)
        with pytest.raises(GvError) as refused:  # pyramid 1: never built
            vis.cull(0, views)
        assert refused.value.code == GV_E_STATE and "view 1" in str(refused.value) and "pyramid 1" in str(refused.value)
        vis.cull(0, [views[0]])
        before = vis.fetch(0, write_back=False, occupancy=sc.count)
        vis.hiz_select(1)
        vis.hiz_build(ps.depth_image(c, 1))
        vis.hiz_drop(1)
        assert code(vis.cull, 0, views) == GV_E_STATE  # dropped
        assert code(vis.cull, 0, [dict(views[0], use_hiz=1 + 7)]) == GV_E_STATE
        after = vis.fetch(0, write_back=False, occupancy=sc.count)  # the pool's previous results are still there
        assert after["draw_count"] == before["draw_count"] > 0 and np.array_equal(after["visible_idx"], before["visible_idx"])
        # use_hiz = 200 behaves as 1: pyramid 0 (selected or not)
        vis.cull(0, [dict(views[0], use_hiz=200)])
        ps.compare_view(vis, oracle, sc.meshes, sc.transforms, sc.entity_to_transform, dict(views[0], use_hiz=200), 0, hz0, "use_hiz 200")
        vis.cull(0, [dict(views[0], use_hiz=200), dict(views[1], use_hiz=0)])
        ps.compare_view(vis, oracle, sc.meshes, sc.transforms, sc.entity_to_transform, dict(views[0], use_hiz=200), 0, hz0, "use_hiz 200, batched")
        # the second phase with a pyramid that is not built
        vis.cull(0, [dict(views[0], use_hiz=0)])
        assert code(vis.cull_second_phase, 0, 1, dict(views[0], use_hiz=3), pool_id=0) == GV_E_STATE


def test_the_second_phase_queries_the_pyramid_its_view_names(state_world, oracle):
    """R \\ S1 over pyramid 2: S1 the first view's records (against pyramid 0), R the oracle's cull of the same view against image 2"""
    sc, c = state_world
    sc = private_copy(sc)
    e2t = sc.entity_to_transform
    view = ps.make_views(c, "1-2")[0]
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.hiz_build(ps.depth_image(c, 0))
        vis.hiz_select(2)
        vis.hiz_build(ps.depth_image(c, 2))
        vis.hiz_select(1)  # (neither of the two)
        vis.cull(0, [dict(view, use_hiz=1)])
        s1 = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, e2t, view, hiz=ps.oracle_pyramid(oracle, c, 0), threads=4)
        r = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, e2t, view, hiz=ps.oracle_pyramid(oracle, c, 2), threads=4)
        vis.cull_second_phase(0, 1, dict(view, use_hiz=3), pool_id=0)
        got = vis.fetch(1, write_back=False, occupancy=sc.count, pool_id=0)
        keep = ~np.isin(r["visible_idx"], s1["visible_idx"])
        want = r["visible_idx"][keep]
        o = np.argsort(want, kind="stable")
        assert 0 < want.size < r["draw_count"]
        assert got["draw_count"] == want.size and np.array_equal(got["visible_idx"], want[o])
        assert np.array_equal(got["baked_model"].view(np.uint32), r["baked_model"][keep][o].view(np.uint32))
        assert np.array_equal(got["distance_sq"].view(np.uint32), r["distance_sq"][keep][o].view(np.uint32))


def test_a_recorded_cull_queries_the_pyramid_it_named_when_it_was_recorded(oracle):
    """gv_cull_batch_begin, two recorded culls with use_hiz = 1, then gv_hiz_select(2) and a build: the recorded culls queried pyramid 0"""
    n = 3001
    c = ps.case("recorded", "gpu", "flat", n, ("1-2",))
    sc = private_copy(ps.build_scene(c))
    other = sc.meshes[:777].copy()
    view = dict(ps.make_views(c, "1-2")[0], use_hiz=1)
    hz0 = ps.oracle_pyramid(oracle, c, 0)
    with GpuVisibility(device=0) as vis:
        vis.bind_transforms(sc.transforms, sc.entity_to_transform)
        vis.bind_pool(0, sc.meshes)
        vis.bind_pool(1, other)
        vis.hierarchy_rebuild()
        vis.hiz_build(ps.depth_image(c, 0))
        vis.sync()
        vis.stats_reset()
        vis.cull_batch_begin()
        vis.cull(0, [view])
        vis.cull(1, [view])
        assert sum(vis.stats()["launches"][k] for k in COUNTED) == 0  # recorded, not launched
        vis.hiz_select(2)
        vis.hiz_build(ps.depth_image(c, 2))
        vis.cull_batch_end()
        ps.compare_view(vis, oracle, sc.meshes, sc.transforms, sc.entity_to_transform, view, 0, hz0, "recorded pool 0", pool_id=0)
        ps.compare_view(vis, oracle, other, sc.transforms, sc.entity_to_transform, view, 0, hz0, "recorded pool 1", pool_id=1)
        # ... and a recorded cull that names pyramid 2 while pyramid 0 is selected again
        vis.hiz_select(0)
        vis.cull_batch_begin()
        vis.cull(0, [dict(view, use_hiz=3)])
        vis.cull(1, [dict(view, use_hiz=1)])
        vis.cull_batch_end()
        ps.compare_view(vis, oracle, sc.meshes, sc.transforms, sc.entity_to_transform, dict(view, use_hiz=3), 0, ps.oracle_pyramid(oracle, c, 2),
                        "recorded, pyramid 2", pool_id=0)
        ps.compare_view(vis, oracle, other, sc.transforms, sc.entity_to_transform, view, 0, hz0, "recorded beside it", pool_id=1)


# ---- 3. images: a pyramid built from a device image reads it ------------------------------------------------------------------------------

def test_three_masks_and_an_occluder_image_alive_at_once():
    import occluders_support as osup
    n = 300
    sc = rs.parity_world(n, seed=7)
    lo, hi = osup.occluder_boxes(sc.meshes, seed=7)
    view = rs.parity_view()
    import occluders_support
    lights = [rs.parity_light(), rs.perspective_light_outside(),
              rs.ortho_light((-0.3, -1.0, 0.2), (0.0, 0.0, occluders_support.CAMERA_BACK), 20.0, 16.0, -400.0, 400.0)]
    sizes = [(64, 48), (37, 23), (64, 48)]
    with GpuVisibility(device=0) as vis:
        bind(vis, sc)
        vis.bind_occluders(0, lo, hi)
        vis.cull(0, [view])
        vis.occluder_begin(48, 32)
        vis.draw_occluders(0, 0, 1)
        vis.hiz_build_from_occluders()  # pyramid 0 reads the occluder image
        pointers = [vis.occluder_depth_device()[0]]
        levels = {0: levels_of(vis, (48, 32))}
        masks = {}
        for k, (light, size) in enumerate(zip(lights, sizes)):
            vis.hiz_select(1 + k)
            vis.receiver_begin(*size)
            vis.draw_receivers(0, 0, light)
            masks[1 + k] = rs.words(vis.receiver_mask()[0]).copy()
            vis.hiz_build_from_receivers()
            pointers.append(vis.receiver_mask_device()[0])
            levels[1 + k] = levels_of(vis, size)
        assert len(set(pointers)) == 4 and all(pointers)
        assert masks[1].tolist() != masks[3].tolist()
        texels = [48 * 32] + [w * h for w, h in sizes]
        for k in (1, 2, 3):  # (the read itself: the words behind a mask's pointer are the mask as it was fetched)
            assert device_words(vis, pointers[k], texels[k]).tolist() == masks[k].ravel().tolist(), k
        occluder_words = device_words(vis, pointers[0], texels[0])
        assert occluder_words.any()
        # a fourth mask, larger than any, and draws into it: the three masks (and the occluder image) are as they were
        vis.hiz_select(4)
        vis.receiver_begin(96, 80)
        fourth = vis.receiver_mask_device()[0]
        assert fourth not in pointers
        vis.draw_receivers(0, 0, lights[0])
        assert np.isfinite(vis.receiver_mask()[0]).any()
        for k in (1, 2, 3):  # every word of the three masks, read where they lie
            assert device_words(vis, pointers[k], texels[k]).tolist() == masks[k].ravel().tolist(), k
        assert device_words(vis, pointers[0], texels[0]).tolist() == occluder_words.tolist()
        for k, size in zip(range(4), [(48, 32)] + sizes):
            vis.hiz_select(k)
            vis.hiz_rebuild()  # from the image the pyramid reads, as it stands now
            assert same_levels(levels_of(vis, size), levels[k]), k
        # with the pyramids dropped the masks are free again (a drop releases the reference, not the image): a begin takes the image
        # of the last begin while no pyramid reads it, then the lowest free one
        for k in range(1, 5):
            vis.hiz_drop(k)
        vis.hiz_select(0)
        vis.receiver_begin(64, 48)
        assert vis.receiver_mask_device()[0] == fourth
        vis.draw_receivers(0, 0, lights[0])
        vis.hiz_build_from_receivers()  # pyramid 0 moves from the occluder image to this mask
        vis.receiver_begin(64, 48)
        assert vis.receiver_mask_device()[0] == pointers[1]
        vis.occluder_begin(48, 32)
        assert vis.occluder_depth_device()[0] == pointers[0]  # ... and the occluder image nobody reads any more is taken again


# ---- 4. end to end: a main pass and three masked cascades in one cull -------------------------------------------------------------------------

SLICES = (60.0, 150.0, rs.SLICE_FAR)


@functools.lru_cache(maxsize=None)
def cascade_lights():
    return tuple(rs.slice_light(np.eye(3), rs.FOV_Y, rs.ASPECT, 0.1, far, rs.LIGHT_DIR)[0] for far in SLICES)


def cascade(k, use_hiz):
    return scene.make_view(cascade_lights()[k], camera_position=rs.CAMERA, shadow_pass=k, use_hiz=use_hiz)


def test_one_cull_of_main_and_three_masked_cascades_equals_the_one_at_a_time_order(oracle):
    sc, _slots = rs.shadow_world()
    n = sc.count
    boxes = rs.aabbs_by_slot(sc.meshes)
    main_view = rs.shadow_views()[0]
    width, height = rs.SHADOW_MASK
    # the oracle: the twin's masks of the main view's records, each cascade against the pyramid of its own
    main = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, main_view)
    want = []
    for k in range(3):
        image, _ = rs.expected(rs.shared_twin(), main, boxes, cascade_lights()[k], width, height)
        want.append(oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, cascade(k, 1), hiz=oracle.Hiz(image)))

    def listed(f):
        return f["visible_idx"][:int(f["draw_count"])].tolist(), f["baked_model"].view(np.uint32).tolist()

    with GpuVisibility(device=0) as vis:  # one batched call
        bind(vis, sc)
        vis.cull(0, [main_view])
        for k in range(3):
            vis.hiz_select(1 + k)
            vis.receiver_begin(width, height)
            vis.draw_receivers(0, 0, cascade_lights()[k])
            vis.hiz_build_from_receivers()
        vis.hiz_select(0)
        vis.stats_reset()
        vis.cull(0, [main_view] + [cascade(k, 2 + k) for k in range(3)])
        assert vis.stats()["launches"]["cull"] == 1
        batched = [vis.fetch(1 + k, write_back=False, occupancy=n, order="slot") for k in range(3)]
        got_main = vis.fetch(0, write_back=False, occupancy=n, order="slot")
    with GpuVisibility(device=0) as vis:  # the existing order: one pyramid, one cascade at a time, the main view named again
        bind(vis, sc)
        vis.cull(0, [main_view])
        single = []
        for k in range(3):
            vis.receiver_begin(width, height)
            vis.draw_receivers(0, 0, cascade_lights()[k])
            vis.hiz_build_from_receivers()
            vis.cull(0, [main_view, cascade(k, 1)])
            single.append(vis.fetch(1, write_back=False, occupancy=n, order="slot"))
    assert listed(got_main)[0] == np.sort(main["visible_idx"]).tolist()
    plain = oracle.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, cascade(2, 0))["draw_count"]
    for k in range(3):
        o = np.argsort(want[k]["visible_idx"], kind="stable")
        expected = (want[k]["visible_idx"][o].tolist(), want[k]["baked_model"][o].view(np.uint32).tolist())
        assert listed(batched[k]) == listed(single[k]), k
        assert listed(batched[k]) == expected, k
        assert int(batched[k]["draw_count"]) > 0
    assert int(batched[2]["draw_count"]) <= int(plain) - 100  # (the mask drops casters the frustum keeps)
