"""The receiver-mask rule of DESIGN.md §4 item 17 on the CPU: known answers of the C twin (tests/receiver_twin.h) that can be derived
by hand, and the end-to-end shadow scene of tests/test_gpu_receivers.py held to its conditions and to the geometry with the oracle's
cull over the twin's mask — so that what the device is compared with is itself checked, and the scene cannot pass vacuously."""
import math

import numpy as np
import pytest

import occluders_support as osup
import receivers_support as rs
from garden_amd import scene


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return rs.build_twin(tmp_path_factory.mktemp("receiver_twin"))


@pytest.fixture(scope="module")
def inner_twin(tmp_path_factory):
    return osup.build_twin(tmp_path_factory.mktemp("occluder_twin"))


# an axis-aligned light looking down +z from the origin: 8 x 8 units wide, depth 0 .. 16; 64 x 64 texels, so 8 texels per unit:
# u = 0.5 + x / 8, v = 0.5 - y / 8, depth = (16 - z) / 16 — all exact in fp32 for the dyadic inputs below
AXIS_LIGHT = rs._cm(rs.ortho_rev_z(-4.0, 4.0, -4.0, 4.0, 0.0, 16.0))
W = H = 64


def bits(x):
    return int(np.float32(x).view(np.uint32))


def test_an_axis_aligned_box_touches_its_rectangle_grown_by_the_margin_and_writes_its_far_face(twin):
    # x 0.0625 .. 1.8125 -> 32.5 .. 46.5 texels (X = 520 .. 744); y -0.75 .. 1.25 -> 22 .. 38 texels (Y = 352 .. 608); z 7 .. 9
    model = osup.model_of((0.9375, 0.25, 8.0), (0.875, 1.0, 1.0))
    s = rs.twin_setup(twin, model, osup.UNIT_BOX, AXIS_LIGHT, W, H)
    assert s["cls"] == rs.DRAWN
    assert sorted(set(s["X"].tolist())) == [520, 744] and sorted(set(s["Y"].tolist())) == [352, 608]
    # step 5: (520 - 2) >> 4 = 32, (744 + 2) >> 4 = 46; (352 - 2) >> 4 = 21 (the box ends ON the texel line 22: the texel above
    # touches it, and the margin keeps it), (608 + 2) >> 4 = 38
    assert s["range"] == (32, 46, 21, 38)
    cls, touched = rs.twin_pixels(twin, model, osup.UNIT_BOX, AXIS_LIGHT, W, H)
    want = np.zeros((H, W), bool)
    want[21:39, 32:47] = True
    assert cls == rs.DRAWN and (touched == want).all()
    image, counts = rs.twin_draw(twin, [model], [osup.UNIT_BOX], AXIS_LIGHT, W, H)
    assert counts == dict(drawn=1, flat=0, behind=0, range=0, outside=0, reserved=0)
    assert bits(s["d"]) == bits(0.4375)  # the far face, z = 9: (16 - 9) / 16
    assert (rs.words(image)[want] == bits(0.4375)).all() and (rs.words(image)[~want] == rs.INF_WORD).all()


def test_a_box_turned_by_45_degrees_touches_less_than_its_range_and_more_than_the_inner_rule_covers(twin, inner_twin):
    model = osup.model_of((0.3, -0.2, 8.0), (1.5, 1.5, 0.5), (0.0, 0.0, math.sin(math.pi / 8), math.cos(math.pi / 8)))
    s = rs.twin_setup(twin, model, osup.UNIT_BOX, AXIS_LIGHT, W, H)
    cls, touched = rs.twin_pixels(twin, model, osup.UNIT_BOX, AXIS_LIGHT, W, H)
    x0, x1, y0, y1 = s["range"]
    in_range = (x1 - x0 + 1) * (y1 - y0 + 1)
    inner, inner_counts = osup.twin_draw(inner_twin, [model], [osup.UNIT_BOX], AXIS_LIGHT, W, H)
    covered = inner != 0
    assert cls == rs.DRAWN and inner_counts["drawn"] == 1 and len(s["edges"]) == 4
    assert 0 < covered.sum() < touched.sum() < in_range
    assert touched[covered].all()  # the outer set holds the inner one
    # the diamond's area is 2 * (1.5 * sqrt(2) * 8)^2 / 2 ... = (3 * 8)^2 = 576 texels: the two rules bracket it
    assert covered.sum() < 576 < touched.sum()


def test_an_edge_on_plate_of_no_thickness_is_flat_and_fills_its_range(twin):
    plate = np.array([-1, 0, -1, 1, 0, 1], np.float32)  # in the xz plane; the light looks along z: a segment on the mask
    model = osup.model_of((0.0, 1.03, 8.0), (2.0, 1.0, 1.0))
    s = rs.twin_setup(twin, model, plate, AXIS_LIGHT, W, H)
    cls, touched = rs.twin_pixels(twin, model, plate, AXIS_LIGHT, W, H)
    assert cls == rs.FLAT and s["edges"] == []
    x0, x1, y0, y1 = s["range"]
    assert (x0, x1) == (15, 48) and y0 == y1 == 23  # v = 0.5 - 1.03 / 8: 23.76 texels
    assert touched.sum() == 34 and touched[23, 15:49].all()
    assert bits(s["d"]) == bits(0.4375)


def test_a_sub_pixel_box_is_flat_or_drawn_and_writes_the_pixel_it_lies_in(twin):
    model = osup.model_of((0.33, 0.41, 5.0), (0.001, 0.001, 0.001))
    cls, touched = rs.twin_pixels(twin, model, osup.UNIT_BOX, AXIS_LIGHT, W, H)
    assert cls in (rs.FLAT, rs.DRAWN) and touched.sum() == 1 and touched[int(32 - 0.41 * 8), int(32 + 0.33 * 8)]


def test_a_perspective_light_with_a_corner_behind_it_gives_a_whole_image_of_plus_zero(twin):
    light = osup.camera(1.0)
    model = osup.model_of((0.0, 0.0, 0.5))  # z from -0.5 to 1.5: straddles w = 0
    image, counts = rs.twin_draw(twin, [model], [osup.UNIT_BOX], light, 37, 23)
    assert counts["behind"] == 1 and sum(counts.values()) == 1
    assert (rs.words(image) == 0).all()


def test_a_nan_scale_is_counted_behind_and_gives_a_whole_image_of_plus_zero(twin):
    """every corner of a NaN model is NaN, and so is its w whatever L holds: step 2's !(w > 0) takes it before step 4 can — counted
    behind, +0.0f everywhere. What reaches step 4's `range` is a finite corner too far out, below"""
    model = osup.model_of((0.0, 0.0, 8.0), (np.nan, 1.0, 1.0))
    image, counts = rs.twin_draw(twin, [model], [osup.UNIT_BOX], AXIS_LIGHT, W, H)
    assert counts["behind"] == 1 and sum(counts.values()) == 1 and (rs.words(image) == 0).all()


def test_a_corner_too_far_out_is_counted_range_and_writes_d_into_the_whole_image(twin):
    model = osup.model_of((0.0, 0.0, 8.0), (4.0e4, 1.0, 1.0))  # u * 1024 beyond 2^22
    s = rs.twin_setup(twin, model, osup.UNIT_BOX, AXIS_LIGHT, W, H)
    image, counts = rs.twin_draw(twin, [model], [osup.UNIT_BOX], AXIS_LIGHT, W, H)
    assert s["cls"] == rs.RANGE and counts["range"] == 1 and s["range"] == (0, W - 1, 0, H - 1)
    assert (rs.words(image) == bits(0.4375)).all()


def test_a_receiver_outside_the_image_writes_nothing(twin):
    model = osup.model_of((9.0, 0.0, 8.0))
    image, counts = rs.twin_draw(twin, [model], [osup.UNIT_BOX], AXIS_LIGHT, W, H)
    assert counts["outside"] == 1 and (rs.words(image) == rs.INF_WORD).all()


def test_depths_beyond_either_plane_and_the_negative_zero(twin):
    beyond = osup.model_of((0.0, 0.0, 20.0))     # behind the far plane: m < 0 -> +0.0f
    in_front = osup.model_of((0.0, 0.0, -3.0))   # in front of the near plane: no upper clamp
    for model, want in ((beyond, 0.0), (in_front, (16.0 + 2.0) / 16.0)):
        s = rs.twin_setup(twin, model, osup.UNIT_BOX, AXIS_LIGHT, W, H)
        assert s["cls"] == rs.DRAWN and bits(s["d"]) == bits(want)
    # m = -0.0f exactly: a depth row of negative zeros over a box in the positive octant (every product is -0.0f, and so is every sum)
    light = AXIS_LIGHT.copy()
    light[[2, 6, 10, 14]] = np.float32(-0.0)
    s = rs.twin_setup(twin, osup.model_of((1.5, 1.5, 8.0)), osup.UNIT_BOX, light, W, H)
    assert [bits(z) for z in s["z"]] == [0x80000000] * 8 and bits(s["d"]) == 0
    models, boxes = osup.census_boxes(3000, 7)
    image, counts = rs.twin_draw(twin, models, boxes, AXIS_LIGHT, W, H)
    assert counts["drawn"] > 100 and not (rs.words(image) >> 31).any()
    assert (rs.words(image) <= rs.INF_WORD).all()


def test_two_overlapping_receivers_give_the_same_words_in_both_orders(twin):
    a = osup.model_of((0.5, 0.0, 6.0), (1.5, 1.0, 1.0), (0.0, 0.0, 0.2, 0.98))
    b = osup.model_of((-0.25, 0.4, 11.0), (2.0, 0.7, 1.0), (0.1, 0.0, -0.3, 0.95))
    ab, counts_ab = rs.twin_draw(twin, [a, b], [osup.UNIT_BOX] * 2, AXIS_LIGHT, W, H)
    ba, counts_ba = rs.twin_draw(twin, [b, a], [osup.UNIT_BOX] * 2, AXIS_LIGHT, W, H)
    only_a, _ = rs.twin_draw(twin, [a], [osup.UNIT_BOX], AXIS_LIGHT, W, H)
    only_b, _ = rs.twin_draw(twin, [b], [osup.UNIT_BOX], AXIS_LIGHT, W, H)
    assert counts_ab == counts_ba and rs.words(ab).tolist() == rs.words(ba).tolist()
    both = np.isfinite(only_a) & np.isfinite(only_b)
    assert both.sum() > 50 and (ab[both] == only_b[both]).all()  # b is farther from the light: its smaller depth stands
    assert rs.words(ab).tolist() == np.minimum(rs.words(only_a), rs.words(only_b)).tolist()


def test_the_parity_cases_reach_both_forms_of_the_setup_launch_and_every_tile_path(twin):
    """over the oracle's records (every slot is a draw of parity_view), per image size: the forms the device's launches take"""
    from oracle import oracle_py
    sc = rs.parity_world(257)
    got = oracle_py.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, rs.parity_view())
    assert int(got["draw_count"]) == 257
    boxes = rs.aabbs_by_slot(sc.meshes)
    seen = {}
    for width, height in rs.IMAGE_SIZES:
        if width <= 512:  # (the census goes pixel by pixel: the largest mask is left to the parity run itself)
            seen[(width, height)] = rs.forms(twin, got, boxes, rs.parity_light(), width, height)
        _, counts = rs.expected(twin, got, boxes, rs.parity_light(), width, height)
        assert counts["drawn"] > 50 and counts["flat"] > 3 and counts["outside"] > 20, (width, height, counts)
    assert seen[(1, 1)]["listed"] == 0 and seen[(1, 1)]["small"] > 100
    for size in ((2 * rs.T + 1, 2 * rs.T + 1), (512, 256)):
        f = seen[size]
        assert f["small"] > 5 and f["listed"] > 20 and f["tiles_all"] > 20 and f["tiles_some"] > 20 and f["tiles_none"] > 0, (size, f)
    # whole-mask records go through the item walk as a full-screen box: the perspective lights, over the world of the GPU case
    sc = rs.parity_world(257, seed=3)
    got = oracle_py.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, rs.parity_view())
    boxes = rs.aabbs_by_slot(sc.meshes)
    for light in (rs.perspective_light_inside(), rs.perspective_light_outside()):
        f = rs.forms(twin, got, boxes, light, 65, 65)
        _, counts = rs.expected(twin, got, boxes, light, 65, 65)
        assert counts["behind"] > 0 and f["tiles_whole_mask"] == 9 * counts["behind"] + 9 * counts["range"]
    _, counts = rs.expected(twin, got, boxes, rs.perspective_light_outside(), 65, 65)
    assert 0 < counts["behind"] < 25 and counts["drawn"] > 100


# ---- the end-to-end shadow scene, on the CPU ------------------------------------------------------------------------------------------

def dropped_and_kept(e):
    plain, masked = set(np.asarray(e["plain"]["visible_idx"]).tolist()), set(np.asarray(e["masked"]["visible_idx"]).tolist())
    assert masked <= plain
    return sorted(plain - masked), sorted(masked)


@pytest.mark.parametrize("rg16f", (False, True))
def test_the_shadow_scene_meets_its_conditions_and_the_planted_casters_fare_as_planned(rg16f):
    e = rs.shadow_oracle(rg16f)
    sc, slots = rs.shadow_world()
    dropped, kept = dropped_and_kept(e)
    main = set(np.asarray(e["main"]["visible_idx"]).tolist())
    assert len(dropped) >= 100 and len(kept) >= 1000 and len(main) >= 1000
    assert slots["floor"] in main and slots["floor"] in kept
    for name, slot in slots.items():
        if name == "floor":
            continue
        assert slot not in main, name          # beside the main frustum: no receiver itself
        assert slot in dropped or slot in kept, name  # ... and inside the cascade
        assert (slot in kept) == name.startswith("above_floor"), name
    # self-keeping: what the main view sees and the cascade's frustum holds survives the masked cull
    plain = set(np.asarray(e["plain"]["visible_idx"]).tolist())
    assert len(main & plain) >= 1000 and (main & plain) <= set(kept)
    # every texel within 8 of an off_floor caster's footprint is +inf
    _, light, _, _ = rs.shadow_views()
    width, height = rs.SHADOW_MASK
    plain_slots, plain_models = rs.records(e["plain"])
    boxes = rs.aabbs_by_slot(sc.meshes)
    for name in ("off_floor_0", "off_floor_1"):
        k = int(np.nonzero(plain_slots == slots[name])[0][0])
        s = rs.twin_setup(rs.shared_twin(), plain_models[k], boxes[slots[name]], light, width, height)
        x0, x1, y0, y1 = s["range"]
        assert s["cls"] in (rs.DRAWN, rs.FLAT) and x0 >= 10 and y0 >= 10 and x1 < width - 10 and y1 < height - 10, (name, s["range"])
        assert (rs.words(e["image"][y0 - 8:y1 + 9, x0 - 8:x1 + 9]) == rs.INF_WORD).all(), name


def test_no_ray_from_a_visible_receiver_towards_the_light_hits_a_dropped_caster():
    e = rs.shadow_oracle(False)
    sc, slots = rs.shadow_world()
    _, light, _, _ = rs.shadow_views()
    width, height = rs.SHADOW_MASK
    boxes = rs.aabbs_by_slot(sc.meshes)
    dropped, kept = dropped_and_kept(e)
    points = rs.sample_points(e["main"], boxes, light, width, height, floor_slot=slots["floor"])
    assert len(points) == 4096
    towards_light = -np.asarray(rs.LIGHT_DIR, np.float64) / np.linalg.norm(rs.LIGHT_DIR)
    plain_slots, plain_models = rs.records(e["plain"])
    model_of_slot = {int(s): plain_models[k] for k, s in enumerate(plain_slots)}
    hits_dropped = rs.rays_hit(points, towards_light, [model_of_slot[s] for s in dropped], boxes[dropped], light)
    assert not hits_dropped.any(), int(hits_dropped.sum())
    some_kept = [s for s in kept if s != slots["floor"]][:2000]
    hits_kept = rs.rays_hit(points, towards_light, [model_of_slot[s] for s in some_kept], boxes[some_kept], light)
    assert hits_kept.sum() >= 100
