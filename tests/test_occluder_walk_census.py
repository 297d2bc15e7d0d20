"""Census of the occluder launches' walks, on the CPU: walk_census (tests/occluders_support.py) restates how occluder_setup_kernel,
occluder_scan_kernel and occluder_raster_kernel (garden_amd/csrc/gv_occluders.hip) divide a set of records among workgroups, scan
turns and waves, and counts the forms a draw takes: rows reused inside a walk, crossings from one occluder to the next (over
records without tiles, over record-block edges, over whole empty blocks), walks that start in the middle of an occluder and of a
tile row, the three tile paths, clipped and cut tiles, half-used wave steps, scan turns, workgroups beyond the count, overlap.

Every case of WALK_CASES (run on the device by tests/test_gpu_occluder_walks.py) must reach the forms it is named for — over the
oracle's records, which are in slot order, and over the same records in the mirror's own order (tests/reorder_support.py). The
conditions are CONDITIONS, not measurements: they keep a case from passing without exercising what it exists for. The older cases
of tests/test_gpu_occluders.py are pinned to what they are: parity at a share of one item per wave."""
import numpy as np
import pytest

import occluders_support as osup
from hiz_paths_support import source_text

ORDERS = ("slot", "mirror")


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return osup.build_twin(tmp_path_factory.mktemp("occluder_twin"))


@pytest.fixture(scope="module")
def censuses(twin):
    """census(name, order, fov): computed once per key"""
    held = {}

    def census(name, order, fov=90.0):
        key = (name, order, fov)
        if key not in held:
            case = osup.WALK_CASE[name]
            records = osup.oracle_records(name, fov)
            if order == "mirror":
                records = osup.mirror_order(name, records)
            models, boxes = osup.records_of(records, osup.walk_world(name)[3])
            held[key] = osup.walk_census(twin, models, boxes, osup.parity_view(fov=fov)["view_proj"], case.width, case.height,
                                         occupancy=case.records)
            print(f"census {name} {order} fov {fov:g}: {osup.census_line(held[key])}")
        return held[key]

    return census


def test_the_kernels_still_read_as_restated():
    for name, lines in osup.WALK_LINES.items():
        text = source_text(name)
        for line in lines:
            assert line in text, f"{name} no longer holds `{line}`: the launches changed, restate walk_census"
    # (the sizes of WALK_CASES were chosen for these values)
    assert (osup.T, osup.BLOCK, osup.RASTER_GROUPS, osup.RASTER_WAVES, osup.SCAN_TURN_BLOCKS) == (32, 256, 1024, 4096, 1024)
    assert len({case.name for case in osup.WALK_CASES}) == len(osup.WALK_CASES) == 7
    assert osup.WALK_CASE["scan-3-turns"].records == 2 * 1024 * osup.BLOCK + 1


def test_the_census_of_a_hand_worked_draw(twin):
    """tests/test_occluder_twin.py works the range of its facing box out by hand: pixels 22 .. 41 x 27 .. 36 of 64 x 64. Two tile
    columns and two tile rows, every tile clipped on two sides; 4 items, a share of 1, no step of the walk beyond the first. The range
    ends at row 36 = 32 + 4 (an even offset: the last step of the lower tiles has its upper row only) and starts at row 27 (odd:
    the first step of the upper tiles has its lower row only). The same box twice around a record without one: 8 items, two occluders over a pixel."""
    model, box = osup.model_of((0.0, 0.0, 8.0), (2.0, 1.0, 1.0)), osup.UNIT_BOX
    vp = osup.camera(aspect=1.0)
    c = osup.walk_census(twin, [model], [box], vp, 64, 64, occupancy=600)
    assert (c["total"], c["share"], c["waves_with_items"], c["last_walk"], c["last_walk_short"]) == (4, 1, 4, 1, False)
    assert (c["reuse"], c["cross"], c["mid_starts"], c["mid_row_starts"], c["single_occluder_walks"]) == (0, 0, 3, 2, 0)
    assert (c["tiles_x_max"], c["tile_rows_max"]) == (2, 2)
    assert (c["clip_left"], c["clip_right"], c["clip_top"], c["clip_bottom"]) == (2, 2, 2, 2)
    assert (c["cut_right_edge"], c["cut_bottom_edge"], c["half_last_step"], c["half_first_step"]) == (0, 0, 2, 2)
    assert (c["inside"], c["mixed"], c["outside"]) == (0, 4, 0) and c["overlap_max"] == 1
    assert (c["scan_turns"], c["drawn_per_turn"], c["setup_grid"], c["blocks_beyond_count"]) == (1, (1,), 3, 2)
    assert (c["block_first_drawn"], c["block_last_drawn"], c["empty_blocks_between"]) == (1, 1, 0)
    c = osup.walk_census(twin, [model] * 3, [box, np.zeros(6, np.float32), box], vp, 64, 64)
    assert (c["total"], c["share"], c["overlap_max"], c["counts"]["drawn"], c["counts"]["no_box"]) == (8, 1, 2, 2, 1)
    # ... and a made-up share: with 4 096 waves, 64 plates of 128 tiles each are two items a wave, every pair inside one plate
    name = "stack"
    models, boxes = osup.records_of(osup.oracle_records(name), osup.walk_world(name)[3])
    c = osup.walk_census(twin, models, boxes, osup.parity_view()["view_proj"], 512, 256)
    assert (c["total"], c["share"], c["reuse"], c["cross"], c["mid_starts"], c["mid_row_starts"]) == (8192, 2, 4096, 0, 4096 - 64, 4096 - 64 * 8)
    assert (c["inside"], c["single_occluder_walks"], c["tiles_x_max"], c["tile_rows_max"]) == (8192, 4096, 16, 8)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("case", osup.WALK_CASES, ids=repr)
def test_every_case_reaches_the_forms_it_exists_for(case, order, censuses):
    records = osup.oracle_records(case.name)
    assert int(records["draw_count"]) == case.records  # (every slot is a draw)
    if order == "slot":
        assert np.asarray(records["visible_idx"]).tolist() == list(range(case.records))
    else:
        delivered = osup.mirror_order(case.name, records)["visible_idx"]
        assert sorted(delivered.tolist()) == list(range(case.records))
        assert (delivered.tolist() == list(range(case.records))) == (case.name == "sparse-then-dense")
    missed = case.missed(censuses(case.name, order))
    assert not missed, f"{case.name} in {order} order no longer reaches: {missed}"
    if case.narrow:
        narrow = censuses(case.name, order, osup.NARROW_FOV)
        missed = case.missed(narrow, case.narrow)
        assert not missed, f"{case.name} in {order} order, narrow view, no longer reaches: {missed}"


def test_the_stack_holds_the_nearest_plates_depth_everywhere(twin):
    name = "stack"
    sc, _, _, by_slot = osup.walk_world(name)
    models, boxes = osup.records_of(osup.oracle_records(name), by_slot)
    vp = osup.parity_view()["view_proj"]
    image, counts = osup.twin_draw(twin, models, boxes, vp, 512, 256)
    depths = [osup.twin_setup(twin, m, b, vp, 512, 256)["d"] for m, b in zip(models, boxes)]
    assert len(set(float(d) for d in depths)) == osup.STACK_PLATES == counts["drawn"]
    nearest = int(np.argmin(sc.transforms["position"][:, 2]))
    assert depths[nearest] == max(depths) and (osup.words(image) == osup.words(np.float32(depths[nearest]))).all()
    assert (np.diff(sc.transforms["position"][:, 2]) < 0).any() and (np.diff(sc.transforms["position"][:, 2]) > 0).any()


def test_the_older_cases_all_walk_one_item_a_wave(twin):
    """What this file rests on: the parity cases of tests/test_gpu_occluders.py take a share of 1 — a wave has at most one item, so
    nothing of a walk beyond its first item runs in them. Whoever enlarges those cases finds here which cases have become redundant."""
    from oracle import oracle_py
    view = osup.parity_view()
    largest = 0
    for n in osup.RECORD_COUNTS:
        sc = osup.parity_world(n)
        lo, hi = osup.occluder_boxes(sc.meshes)
        records = oracle_py.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, view)
        models, boxes = osup.records_of(records, osup.boxes_by_slot(lo, hi))
        for width, height in osup.IMAGE_SIZES:
            c = osup.walk_census(twin, models, boxes, view["view_proj"], width, height)
            assert c["share"] <= 1 and c["reuse"] == c["cross"] == 0 and c["scan_turns"] == 1, (n, width, height, c)
            largest = max(largest, c["total"])
    assert 0 < largest <= osup.RASTER_WAVES
    # the mirror-order test's world reaches two items a wave, and no more
    sc = osup.parity_world(3000, seed=5)
    lo, hi = osup.occluder_boxes(sc.meshes, seed=5)
    records = oracle_py.prepare_meshes(sc.meshes.copy(), sc.transforms, sc.entity_to_transform, view)
    models, boxes = osup.records_of(records, osup.boxes_by_slot(lo, hi))
    assert osup.walk_census(twin, models, boxes, view["view_proj"], 64, 48)["share"] == 2


def test_the_cases_between_them_reach_every_field_of_the_census(censuses):
    """the census is not vacuous: every count it returns is above zero in some case and order, and both answers of its one flag occur"""
    seen = [censuses(case.name, order) for case in osup.WALK_CASES for order in ORDERS]
    seen += [censuses(case.name, order, osup.NARROW_FOV) for case in osup.WALK_CASES if case.narrow for order in ORDERS]
    fields = set(seen[0]) - {"counts", "drawn_per_turn", "last_walk_short"}
    assert len(fields) == 34 and all(set(c) == set(seen[0]) for c in seen)
    never = sorted(f for f in fields if not any(c[f] > 0 for c in seen))
    assert not never, f"no case reaches: {never}"
    assert {c["last_walk_short"] for c in seen} == {False, True}
    assert max(len(c["drawn_per_turn"]) for c in seen) == 3 and max(c["share"] for c in seen) >= 16
    # in the thousands, as the device tests are meant to run them: every tile path, reuse, mid-row starts; crossings in the hundreds
    for field, least in (("inside", 10_000), ("mixed", 10_000), ("outside", 10_000), ("reuse", 50_000), ("mid_row_starts", 3000), ("cross", 500),
                         ("cross_over_empty", 50), ("tiles_x_max", 65), ("overlap_max", 64), ("half_last_step", 1000), ("blocks_beyond_count", 1024)):
        assert max(c[field] for c in seen) >= least, field
    for name in ("behind", "no_box", "flat", "small", "drawn"):
        assert any(c["counts"][name] > 0 for c in seen), name
