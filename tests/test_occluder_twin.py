"""The occluder-depth rule on the CPU tier, through its C twin (tests/occluder_twin.h): known answers worked out
by hand, one case per skip class, and the conservativeness census — the twin's coverage of 20 000 random boxes per image size held
to the float64 convex hull of the float64 projection: no written pixel may have a corner outside it at the rule's margin, and the
same census must find violations at margin 0 (so it cannot pass vacuously)."""
import numpy as np
import pytest

import occluders_support as osup

F32 = np.float32
CENSUS_BOXES = 20_000


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return osup.build_twin(tmp_path_factory.mktemp("occluder_twin"))


SQUARE = osup.camera(aspect=1.0)  # clip x = x, clip y = -y, w = z, clip z = 0.01


def facing_box():
    """x in [-2, 2], y in [-1, 1], z in [7, 9] in front of SQUARE"""
    return osup.model_of((0.0, 0.0, 8.0), (2.0, 1.0, 1.0)), osup.UNIT_BOX


def test_a_box_facing_the_camera_covers_the_hand_computed_rectangle(twin):
    """64 x 64: the front face (z = 7) spans u = .5 -+ 1/7, v = .5 -+ 1/14, the back face projects inside it. In sixteenths of a
    pixel: X = floor(365.71) = 365 .. floor(658.29) = 658, Y = 438 .. 585. An axis-aligned edge asks for a distance of 2 units, so
    a pixel corner passes inside [367, 656] x [440, 583]: cx = 23 .. 41, cy = 28 .. 36, pixels 23 .. 40 x 28 .. 35. The depth is the
    back face's: 0.01 * (1 / 9)."""
    model, box = facing_box()
    s = osup.twin_setup(twin, model, box, SQUARE, 64, 64)
    assert s["cls"] == osup.DRAWN
    assert (int(s["X"].min()), int(s["X"].max()), int(s["Y"].min()), int(s["Y"].max())) == (365, 658, 438, 585)
    assert s["range"] == (22, 41, 27, 36)
    image, counts = osup.twin_draw(twin, [model], [box], SQUARE, 64, 64)
    want = np.zeros((64, 64), F32)
    want[28:36, 23:41] = F32(0.01) * (F32(1.0) / F32(9.0))
    assert osup.words(image).tolist() == osup.words(want).tolist()
    assert counts == dict(drawn=1, no_box=0, behind=0, range=0, flat=0, small=0)


def test_face_on_has_four_active_edges_and_corner_on_six(twin):
    model, box = facing_box()
    s = osup.twin_setup(twin, model, box, SQUARE, 64, 64)
    assert len(s["edges"]) == 4 and sum(s["positive"]) == 1
    # the four edges are one face's cycle: every corner is left once and entered once
    assert sorted(a for a, _ in s["edges"]) == sorted(b for _, b in s["edges"]) and len({a for a, _ in s["edges"]}) == 4
    # looked at along its diagonal, three faces face the camera: six silhouette edges in one closed cycle
    diagonal = osup.model_of((0.0, 0.0, 8.0), (1.0, 1.0, 1.0), (0.32505758, -0.32505758, 0.0, 0.88807383))  # turns (1,1,1) onto the z axis
    s = osup.twin_setup(twin, diagonal, osup.UNIT_BOX, SQUARE, 64, 64)
    assert s["cls"] == osup.DRAWN and len(s["edges"]) == 6 and sum(s["positive"]) == 3
    follow = dict(s["edges"])
    at, seen = s["edges"][0][0], []
    for _ in range(6):
        seen.append(at)
        at = follow[at]
    assert at == seen[0] and len(set(seen)) == 6


def test_a_mirrored_box_gives_the_image_of_its_unmirrored_twin(twin):
    quat = (0.2, -0.3, 0.1, 0.9273618)
    images = []
    for sx in (1.5, -1.5):
        model = osup.model_of((1.0, -0.5, 6.0), (sx, 0.8, 2.0), quat)
        s = osup.twin_setup(twin, model, osup.UNIT_BOX, SQUARE, 96, 64)
        assert s["cls"] == osup.DRAWN
        images.append((osup.twin_draw(twin, [model], [osup.UNIT_BOX], SQUARE, 96, 64)[0], s))
    assert np.count_nonzero(images[0][0]) > 50
    assert osup.words(images[0][0]).tolist() == osup.words(images[1][0]).tolist()
    assert images[0][1]["positive"] != images[1][1]["positive"]  # (the other set of faces bounds the same silhouette)
    # ... and a mirrored projection draws as many pixels as the plain one, give or take the floor's asymmetry
    flipped = osup.twin_draw(twin, [osup.model_of((1.0, -0.5, 6.0), (1.5, 0.8, 2.0), quat)], [osup.UNIT_BOX],
                             osup.camera(aspect=1.0, mirrored=True), 96, 64)[0]
    assert abs(np.count_nonzero(flipped) - np.count_nonzero(images[0][0])) <= 40 and np.count_nonzero(flipped) > 50


@pytest.mark.parametrize("name", sorted(osup.SKIP_TRS) + ["behind_far"])
def test_each_skip_class_increments_exactly_its_count_and_draws_nothing(name, twin):
    position, scale, box = osup.SKIP_TRS["drawn" if name == "behind_far" else name]
    model, box = osup.model_of(position, scale), np.array(box, F32)
    vp = SQUARE.copy()
    if name == "behind_far":
        vp[14] = -vp[14]  # clip z = -0.01: every depth is negative, !(d > 0)
    field = "no_box" if name.startswith("no_box") else name.split("_")[0]
    min_pixels = 8 if name == "small" else 1
    s = osup.twin_setup(twin, model, box, vp, 64, 64, min_pixels)
    assert osup.COUNT_NAMES[s["cls"]] == field
    image, counts = osup.twin_draw(twin, [model], [box], vp, 64, 64, min_pixels)
    assert counts == {k: int(k == field) for k in osup.COUNT_NAMES}
    assert image.any() == (field == "drawn")


def test_small_depends_on_min_pixels(twin):
    model = osup.model_of((0, 0, 20), (1.0, 1.0, 1.0))  # about 3 pixels across at 64 x 64
    assert osup.twin_setup(twin, model, osup.UNIT_BOX, SQUARE, 64, 64, 1)["cls"] == osup.DRAWN
    assert osup.twin_setup(twin, model, osup.UNIT_BOX, SQUARE, 64, 64, 8)["cls"] == osup.SMALL


def test_a_box_equal_to_the_aabb_stores_no_more_than_the_querys_znear(twin):
    """Against the ORACLE's Hi-Z query (gvo_hiz_occluded), probed through its answer over constant depth images: it answers
    "occluded" iff zNear < zFar, so over an image that holds D everywhere it pins its zNear between two neighbouring floats. The
    twin's z words are the query's own: the query's zNear is exactly their maximum — not occluded at D = max z, occluded one float
    above — and over an image that holds the twin's d, what the box itself would draw, the box is not occluded."""
    from oracle import oracle_py
    models, boxes = osup.census_boxes(300, 7)
    vp = osup.camera(96.0 / 64.0)
    pinned = 0
    for model, box in zip(models, boxes):
        s = osup.twin_setup(twin, model, box, vp, 96, 64)
        if s["cls"] != osup.DRAWN:
            continue
        znear = F32(s["z"].max())
        assert s["d"] == min(float(s["z"].min()), 1.0) and s["d"] <= znear
        model4 = np.zeros((4, 4), F32)  # column-major: c0 c1 c2 c3, bottom row (0, 0, 0, 1)
        model4[:, :3] = model.reshape(4, 3)
        model4[3, 3] = 1.0
        answers = [oracle_py.Hiz(np.full((64, 96), depth, F32)).occluded(vp, box[:3], box[3:], model4.reshape(16))
                   for depth in (s["d"], znear, np.nextafter(znear, F32(np.inf)))]
        assert answers == [False, False, True], (answers, s["d"], znear)
        pinned += 1
    assert pinned > 100


def test_every_tile_path_is_taken_by_a_full_screen_occluder_at_two_tiles_plus_one(twin):
    width = height = 2 * osup.T + 1
    model = osup.FULL_SCREEN_PLATE
    inside, mixed, outside = osup.twin_paths(twin, [model], [osup.UNIT_BOX], SQUARE, width, height)
    assert inside >= 1 and mixed >= 1 and outside >= 1 and inside + mixed + outside == 9


@pytest.mark.parametrize("width,height,seed", [(96, 64, 1), (37, 23, 2)])
def test_census_no_written_pixel_leaves_the_float64_hull(width, height, seed, twin):
    models, boxes = osup.census_boxes(CENSUS_BOXES, seed)
    vp = osup.camera(width / height)
    rule = osup.twin_census(twin, models, boxes, vp, width, height, 2)
    loose = osup.twin_census(twin, models, boxes, vp, width, height, 0)
    print(f"census {width}x{height}: margin 2 {rule}; margin 0 {loose}")
    assert rule["drawn"] > CENSUS_BOXES // 4 and rule["unjudged"] == 0
    assert rule["written"] > 20 * rule["drawn"] // 10  # (the census is about covered pixels: it must have some)
    assert rule["violations"] == 0
    assert loose["violations"] > 0 and loose["written"] > rule["written"]
    dets = np.linalg.det(models[:, :9].reshape(-1, 3, 3).astype(np.float64))
    assert (dets < 0).sum() > CENSUS_BOXES // 8 and (dets > 0).sum() > CENSUS_BOXES // 2
