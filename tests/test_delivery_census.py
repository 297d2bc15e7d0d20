"""Census of the results delivery, on the CPU: delivery_plan (tests/delivery_support.py) restates gv_pool_results_fetch's choice
of route, sort_publishes, the flushes of the pending sorts, publish_args_of, deliver_small and deliver_large of
garden_amd/csrc/gv_results.cpp. A search over pool sizes on either side of every handover, the model's flags (mirror permuted,
record layout, emitted or count-only, main or shadow pass, sorted or not), frames of one to three pools and the order of the
fetches collects every reachable CELL (route, records, visibility); the frames of CASES (run by
tests/test_gpu_delivery_forms.py against the oracle) must between them hold each one.

CONDITION, not a measurement: GPU cases hold at most 300 001 entries. Every handover of this path lies at or below 262 145, so no
cell needs pinning to a test beyond that cap: PINNED is empty, and a change of the dispatch that moves a handover beyond the cap
fails here and asks for a pin by name."""
import itertools

import pytest

import delivery_support as ds

SIZE_CAP = 300_001
OCCUPANCIES = (1, 2, 3, 5, 255, 16_383, 16_384, 16_385, 32_767, 32_768, 32_769, 262_143, 262_144, 262_145, 300_001)

# Cells that exist only above SIZE_CAP: cell -> (why, the test that covers it). None: see the module's docstring.
PINNED = {}

# the six kinds of view: emitted or count-only, main or shadow pass, sorted (emitted views only) or not
KINDS = [ds.View(e, m, s) for e, m, s in itertools.product((True, False), (True, False), (0, 1)) if e or not s]
# What a second and a third pool can change for the first, each as one shadow pass with records — a companion's own cells are
# those of a first pool, and whether it is a main pass, count-only or permuted changes nothing for the others:
shadow, sorted_shadow = ds.View(True, False, 0), ds.View(True, False, 1)
COMPANIONS = [
    ds.Pool(255, False, True, (shadow,)),             # an unsorted small view: the sort does not publish
    ds.Pool(255, False, True, (sorted_shadow,)),      # a small sorted list of structs: published by the sort with the others
    ds.Pool(255, False, False, (sorted_shadow,)),     # a small sorted list of arrays: the sort does not publish
    ds.Pool(16_385, False, True, (sorted_shadow,)),   # a mid-sized sorted list: an unpublished small view after its flush
    ds.Pool(262_145, False, True, (shadow,)),         # a large view: beyond the publish launch, keeps nothing from publishing
]


def frames():
    """one pool under one or two views of every kind; the same beside every companion; one pool under one view beside every pair
    of companions. Every set of pools under both orders of the fetches."""
    singles = [(k,) for k in KINDS]
    pairs = [(a, b) for a in KINDS for b in KINDS]
    first = [ds.Pool(occ, perm, layout, views) for occ, perm, layout, views in
             itertools.product(OCCUPANCIES, (False, True), (False, True), singles + pairs)]
    for a in first:
        yield (a,)
        for b in COMPANIONS:
            yield (a, b)
    for a in first:
        if len(a.views) == 1:
            for b, c in itertools.product(COMPANIONS, COMPANIONS):
                yield (a, b, c)


@pytest.fixture(scope="module")
def reachable():
    """{cell: the smallest frame found that takes it, as (occupancy of the view's pool, pools, fetches)}"""
    found = {}
    count = 0
    for pools in frames():
        keys = tuple((p, v) for p, pool in enumerate(pools) for v in range(len(pool.views)))
        for order in (keys, keys[::-1]):
            count += 1
            for (p, _v), cell in ds.delivery_plan(ds.Frame(pools, order)).items():
                size = pools[p].occupancy
                if cell not in found or size < found[cell][0]:
                    found[cell] = (size, pools, order)
    print(f"census: {count} frames searched")
    return found


@pytest.fixture(scope="module")
def held():
    return ds.all_case_cells()


def test_the_dispatch_still_reads_as_restated():
    for name, lines in ds.LITERAL_LINES.items():
        text = ds.source_text(name)
        for line in lines:
            assert line in text, f"{name} no longer holds `{line}`: the delivery changed, restate delivery_plan"
    # (the sizes of CASES and of the record-count edges were chosen for these values)
    assert (ds.BATCH_SORT_MAX, ds.PUBLISH_LDS, ds.PUBLISH_MAX, ds.MAX_PUBLISH_VIEWS, ds.MAX_RECORD_STRIDE) == (16384, 32768, 262144, 32, 128)
    assert ds.PUBLISH_MAX + 1 <= SIZE_CAP < ds.MID_SORT_MAX
    assert max(dt.itemsize for dt, _ in ds.LAYOUTS.values()) == ds.MAX_RECORD_STRIDE


def test_every_reachable_cell_has_a_case(reachable, held):
    for cell in sorted(reachable):
        size, pools, order = reachable[cell]
        print(f"census {str(cell):<36} {'pinned' if cell in PINNED else ('case ' + held[cell] if cell in held else 'MISSING')}; smallest: "
              f"{size} slots, {len(pools)} pool(s), first fetch {order[0]}")
    assert all(r in ds.ROUTES and rec in ds.RECORDS and vis in ds.VISIBILITY for r, rec, vis in reachable)
    missing = sorted(c for c in reachable if c not in PINNED and c not in held)
    assert not missing, f"no case of delivery_support.CASES takes: {missing}"
    unknown = sorted(c for c in held if c not in reachable)
    assert not unknown, f"cells of CASES that the search never found (extend the search): {unknown}"
    # every route in every form it can take: a publishing sort delivers structs only; copies never un-permute in LDS
    assert {c[0] for c in reachable} == set(ds.ROUTES)
    assert {c for c in reachable if c[0] == "sort"} == {("sort", "structs", v) for v in ("lds", "straight", "none")}
    assert {c for c in reachable if c[0] == "publish"} == {("publish", r, v) for r in ds.RECORDS for v in ds.VISIBILITY}
    assert {c for c in reachable if c[0] == "found"} == {("found", r, v) for r in ds.RECORDS for v in ds.VISIBILITY}
    assert {c for c in reachable if c[0] == "copies"} == {("copies", r, v) for r in ds.RECORDS for v in ("device", "straight", "none")}


def test_nothing_needs_pinning_under_the_cap(reachable):
    assert all(where[0] <= SIZE_CAP for where in reachable.values())
    for cell, (why, test) in PINNED.items():
        assert cell in reachable and reachable[cell][0] > SIZE_CAP and why and "::" in test
    for c in ds.CASES:
        assert max(c.sizes) <= SIZE_CAP, c.name
    assert len({c.name for c in ds.CASES}) == len(ds.CASES)


def test_the_handovers_sit_where_the_cases_put_them():
    """one pool, one view, on either side of each handover"""
    def cell(occupancy, permuted, layout, view, other=()):
        plan = ds.delivery_plan(ds.Frame((ds.Pool(occupancy, permuted, layout, (view,)),) + other, ((0, 0),)))
        return plan[(0, 0)]

    sorted_main, main, shadow = ds.View(True, True, 1), ds.View(True, True, 0), ds.View(True, False, 0)
    assert cell(ds.BATCH_SORT_MAX, True, True, sorted_main) == ("sort", "structs", "lds")
    assert cell(ds.BATCH_SORT_MAX + 1, True, True, sorted_main) == ("publish", "structs", "lds")  # behind a mid sort
    assert cell(ds.BATCH_SORT_MAX, True, False, sorted_main) == ("publish", "arrays", "lds")      # arrays leave by the publish launch
    assert cell(ds.PUBLISH_LDS, True, False, main) == ("publish", "arrays", "lds")
    assert cell(ds.PUBLISH_LDS + 1, True, False, main) == ("publish", "arrays", "device")
    assert cell(ds.PUBLISH_LDS + 1, False, False, main) == ("publish", "arrays", "straight")
    assert cell(ds.PUBLISH_MAX, True, True, main) == ("publish", "structs", "device")
    assert cell(ds.PUBLISH_MAX + 1, True, True, main) == ("copies", "structs", "device")
    assert cell(ds.PUBLISH_MAX + 1, False, True, shadow) == ("copies", "structs", "none")
    # an unsorted small view anywhere in the frame keeps the sort from publishing; a large one does not
    beside = lambda n: (ds.Pool(n, False, True, (shadow,)),)
    assert cell(3000, True, True, sorted_main, beside(255)) == ("publish", "structs", "lds")
    assert cell(3000, True, True, sorted_main, beside(ds.PUBLISH_MAX)) == ("publish", "structs", "lds")
    assert cell(3000, True, True, sorted_main, beside(ds.PUBLISH_MAX + 1)) == ("sort", "structs", "lds")


def test_more_views_than_a_batch_take_two_launches():
    """forty unpublished views, pool 2 fetched first: its launch takes pools 2, 3, 4 and 0 — 32 views —, pool 1 waits for a
    fetch of its own, and every other fetch finds its view delivered"""
    for c in ds.CASES:
        if not c.name.startswith("forty-views"):
            continue
        trace = []
        frame = ds.frame_model(c, c.frames[0])
        plan = ds.delivery_plan(frame, trace)
        assert len(plan) == 40 and frame.fetches[0][0] == 2
        launches = [(f, views) for f, what, views in trace if what == "publish"]
        assert [len(views) for _f, views in launches] == [ds.MAX_PUBLISH_VIEWS, 40 - ds.MAX_PUBLISH_VIEWS]
        assert {p for p, _v in launches[0][1]} == {2, 3, 4, 0} and {p for p, _v in launches[1][1]} == {1}
        assert sum(what == "found" for _f, what, _v in trace) == 38


def test_the_sort_publishes_only_in_the_frames_meant_for_it():
    for c in ds.CASES:
        if not c.name.startswith("who-publishes"):
            continue
        routes = []
        for frm in c.frames:
            trace = []
            ds.delivery_plan(ds.frame_model(c, frm), trace)
            routes.append({what for _f, what, _v in trace if what.endswith("sort")})
        assert routes == [{"publishing_sort"}] * 2 + [{"small_sort"}] * 4, c.name
