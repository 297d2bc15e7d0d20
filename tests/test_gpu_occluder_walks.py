"""gv_pool_draw_occluders on the device at the image sizes it is used at: every case of occluders_support.WALK_CASES in both mirror
orders, every word of the image and all six counts equal to the C twin over the records fetched in front of the call. The cases
exist for the forms of the raster and scan launches that the small images of tests/test_gpu_occluders.py leave idle — walks of
many items, crossings between occluders, tile decode on wide tile grids, the inside path by the thousand, scan turns beyond the
first; tests/test_occluder_walk_census.py says which case reaches which form, and every test here takes the census again over the
records the device really delivered. Then the pyramid from a 1000 x 600 image against a second context's pyramid of the twin's
image, the Hi-Z cull against the oracle's over that image, and the second image at 2048 x 1024."""
import numpy as np
import pytest

import hiz_paths_support as hp
import occluders_support as osup
from garden_amd.lib import GpuVisibility
from test_gpu_occluders import bind, fetch

pytestmark = pytest.mark.gpu

ORDERS = (False, True)  # keep_slot_order


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return osup.build_twin(tmp_path_factory.mktemp("occluder_twin"))


def draw_and_compare(vis, twin, draws, width, height, min_pixels=1):
    """draw_and_check of tests/test_gpu_occluders.py for large images: one image; for every (pool, view index, view, boxes by slot,
    occupancy) of `draws` the records are fetched, the twin accumulates them and the device draws them. All six counts and every word
    of the image must agree; a difference is reported by its first pixel and tile. Returns (image, counts, the fetched results)."""
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
    difference = osup.first_difference(got_image, image)
    assert difference is None, difference
    return got_image, got_counts, fetched


def census_of(twin, case, fetched, view, boxes, label, conditions=None):
    """the census over the records the device delivered, printed, and the case's conditions on it"""
    models, by_record = osup.records_of(fetched, boxes)
    census = osup.walk_census(twin, models, by_record, view["view_proj"], case.width, case.height, occupancy=case.records)
    print(f"census {case.name} {label}: {osup.census_line(census)}")
    missed = case.missed(census, conditions)
    assert not missed, f"{case.name}, {label}: the delivered records do not reach: {missed}"
    return census


def label_of(keep_slot_order):
    return "slot order" if keep_slot_order else "mirror order"


def delivered_in(fetched, keep_slot_order, n, mirror_is_slot_order=False):
    order = fetched["visible_idx"][:n].astype(np.int64)
    return bool((np.diff(order) > 0).all()) == (keep_slot_order or mirror_is_slot_order)


def levels_of(vis, width, height):
    sizes = hp.mip_sizes(width, height)
    assert vis.hiz_mip_count() == len(sizes)
    return [vis.hiz_read_level(level, *sizes[level]).view(np.uint32).copy() for level in range(1, len(sizes))]


# ---- 1. bit parity of every case, both mirror orders ------------------------------------------------------------------------------

@pytest.mark.parametrize("keep_slot_order", ORDERS)
@pytest.mark.parametrize("name", ("share-2", "npot-1000x600", "wide-4099x33", "full-2048x1024", "sparse-then-dense"))
def test_every_word_and_count_equals_the_twin_at_size(name, keep_slot_order, twin):
    case = osup.WALK_CASE[name]
    sc, lo, hi, boxes = osup.walk_world(name)
    n = case.records
    view = osup.parity_view()
    with GpuVisibility(device=0, keep_slot_order=keep_slot_order) as vis:
        bind(vis, sc, lo, hi)
        vis.cull(0, [view])
        image, counts, fetched = draw_and_compare(vis, twin, [(0, 0, view, boxes, n)], case.width, case.height)
    assert int(fetched[0]["draw_count"]) == n == sum(counts.values())
    assert delivered_in(fetched[0], keep_slot_order, n, mirror_is_slot_order=name == "sparse-then-dense")
    census = census_of(twin, case, fetched[0], view, boxes, label_of(keep_slot_order))
    assert census["counts"] == counts and np.count_nonzero(image) > case.width * case.height // 4


@pytest.mark.parametrize("keep_slot_order", ORDERS)
def test_a_stack_of_plates_in_three_orders(keep_slot_order, twin):
    """64 plates over every pixel, drawn in raw order, nearest first and farthest first: the maximum does not care, and every pixel
    holds the nearest plate's depth"""
    case = osup.WALK_CASE["stack"]
    sc, lo, hi, boxes = osup.walk_world(case.name)
    n = case.records
    view = osup.parity_view()
    draws = [(0, 0, view, boxes, n)]
    images, orders = [], []
    with GpuVisibility(device=0, keep_slot_order=keep_slot_order) as vis:
        bind(vis, sc, lo, hi)
        for descending in (None, False, True):
            vis.cull(0, [view])
            if descending is not None:
                vis.sort(0, descending=descending, pool_id=0)
            image, counts, fetched = draw_and_compare(vis, twin, draws, case.width, case.height)
            census_of(twin, case, fetched[0], view, boxes, f"{label_of(keep_slot_order)}, {('raw', 'ascending', 'descending')[len(images)]}")
            assert counts["drawn"] == n
            images.append(image)
            orders.append(fetched[0]["visible_idx"][:n].astype(np.int64))
    depth = sc.transforms["position"][:, 2]
    assert (np.diff(depth[orders[1]]) > 0).all() and (np.diff(depth[orders[2]]) < 0).all()  # nearest first, farthest first
    assert not keep_slot_order or orders[0].tolist() == list(range(n))
    assert osup.first_difference(images[1], images[0]) is None and osup.first_difference(images[2], images[0]) is None
    nearest = int(np.argmin(depth))
    d = osup.twin_setup(twin, fetched[0]["baked_model"][orders[2].tolist().index(nearest)], boxes[nearest], view["view_proj"], case.width, case.height)["d"]
    assert (osup.words(images[0]) == osup.words(np.float32(d))).all()


# ---- 2. scan turns and sparse grids -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("keep_slot_order", ORDERS)
def test_three_scan_turns_and_a_grid_mostly_beyond_the_count(keep_slot_order, twin):
    """2 * 1024 * 256 + 1 records, a box on every 509th slot: the scan launch takes three turns, the last for one block of one
    record, which is drawn; then a narrow view of the same pool into the same image, whose count leaves most of the setup grid idle"""
    case = osup.WALK_CASE["scan-3-turns"]
    sc, lo, hi, boxes = osup.walk_world(case.name)
    n = case.records
    wide, narrow = osup.parity_view(), osup.parity_view(fov=osup.NARROW_FOV)
    with GpuVisibility(device=0, keep_slot_order=keep_slot_order) as vis:
        bind(vis, sc, lo, hi)
        vis.cull(0, [wide, narrow])
        image, counts, fetched = draw_and_compare(vis, twin, [(0, 0, wide, boxes, n), (0, 1, narrow, boxes, n)], case.width, case.height)
        alone, _, _ = draw_and_compare(vis, twin, [(0, 0, wide, boxes, n)], case.width, case.height)
    assert int(fetched[0]["draw_count"]) == n and 0 < int(fetched[1]["draw_count"]) < n // 2
    assert sum(counts.values()) == n + int(fetched[1]["draw_count"])
    assert delivered_in(fetched[0], keep_slot_order, n) and delivered_in(fetched[1], keep_slot_order, int(fetched[1]["draw_count"]))
    census_of(twin, case, fetched[0], wide, boxes, label_of(keep_slot_order))
    census_of(twin, case, fetched[1], narrow, boxes, label_of(keep_slot_order) + ", narrow view", case.narrow)
    assert osup.first_difference(alone, image) is not None  # (the second draw added to the image)


# ---- 3. the pyramid from an image at size, and the second image ------------------------------------------------------------------------

def test_the_pyramid_of_a_1000x600_image_and_the_cull_against_it(twin):
    from oracle import oracle_py
    case = osup.WALK_CASE["npot-1000x600"]
    width, height, n = case.width, case.height, case.records
    sc, lo, hi, boxes = osup.walk_world(case.name)
    view, hiz_view = osup.parity_view(), osup.parity_view(use_hiz=1)
    with GpuVisibility(device=0) as vis:
        bind(vis, sc, lo, hi)
        vis.cull(0, [view])
        image, _, _ = draw_and_compare(vis, twin, [(0, 0, view, boxes, n)], width, height)  # (the image IS the twin's, word for word)
        vis.hiz_build_from_occluders()
        levels = levels_of(vis, width, height)
        with GpuVisibility(device=0) as other:
            other.hiz_build(image)
            want_levels = levels_of(other, width, height)
        assert len(levels) == len(want_levels) >= 9
        for level, (got, want) in enumerate(zip(levels, want_levels), start=1):
            assert np.array_equal(got, want), f"level {level}: {int((got != want).sum())} of {got.size} words differ"
        # the cull against that pyramid is the oracle's against the twin's image
        want = oracle_py.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, hiz_view, hiz=oracle_py.Hiz(image))
        assert 0 < int(want["draw_count"]) < n - 20
        vis.cull(0, [hiz_view])
        got = fetch(vis, 0, n, order="slot")
        assert int(got["draw_count"]) == int(want["draw_count"])
        assert np.array_equal(got["visible_idx"], np.asarray(want["visible_idx"]))
        assert np.array_equal(got["baked_model"].view(np.uint32), np.asarray(want["baked_model"], np.float32).view(np.uint32))
        # a new begin takes the OTHER image, at another size: the pyramid's is not cleared or drawn over
        full = osup.WALK_CASE["full-2048x1024"]
        other_image, other_counts, fetched = draw_and_compare(vis, twin, [(0, 0, hiz_view, boxes, n)], full.width, full.height)
        assert other_image.shape == (full.height, full.width) and other_image.any()
        assert int(fetched[0]["draw_count"]) == int(want["draw_count"]) == sum(other_counts.values())
        vis.occluder_begin(width, height)  # (starting over keeps away from the pyramid's image too)
        vis.hiz_rebuild()
        again = levels_of(vis, width, height)
        assert len(again) == len(levels) and all(np.array_equal(a, b) for a, b in zip(again, levels))
        vis.cull(0, [hiz_view])
        assert np.array_equal(fetch(vis, 0, n, order="slot")["visible_idx"], np.asarray(want["visible_idx"]))
