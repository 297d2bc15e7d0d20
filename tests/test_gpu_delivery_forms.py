"""Every form in which results reach the host (gv_pool_results_fetch: the publishing small-pool sort, the publish launch, the
large route's copies, a view found already delivered), against the oracle's prepareMeshes: the frames of
tests/delivery_support.py CASES — which tests/test_delivery_census.py proves to hold every reachable (route, records,
visibility) — and the edges beside the dispatch: record counts at the 64-record chunk and at a whole round of the grids,
record layouts up to 128 bytes with fields out of order and componentOffset values beyond 2^32, records in world slots, record
targets, more views than one publish launch holds.

Every delivered view is compared with oracle.prepare_meshes on a copy of the bound pool, bit for bit: the count, the slots,
baked_model, distance_sq and, for a main pass, the isVisible column the oracle wrote. Unsorted lists are compared ordered by slot
(slots unique); sorted lists must be monotone in distanceSq and are compared with ties canonicalised by slot. No tolerance."""
import functools

import numpy as np
import pytest

import delivery_support as ds
from garden_amd import scene
from test_gpu_sort_forms import box_view, scene_side

COMPONENT_STRIDE = 1 << 20  # componentOffset = slot << 20: beyond 2^32 from slot 4096 on
# records under the whole-cube view of flat(n), checked with the oracle alone
CUBE_RECORDS = {3: 3, 3000: 2900, 16_384: 15_727, 32_769: 31_485, 262_145: 251_803}
CONTEXTS = pytest.mark.parametrize("keep_slot_order", [False, True], ids=["spatial", "slot"])  # isVisible un-permuted / copied as it is


# ---- scenes, views and the oracle's results: built once per module ----

@functools.lru_cache(maxsize=3)
def flat(total, defects=True):
    """scene.flat_scene(total, seed=total + 5), the scenes of test_records_in_the_engines_own_struct_layout: CUBE_RECORDS holds for them"""
    return scene.flat_scene(total, seed=total + 5, defects=defects)


def camera(j, side, main=True, emitted=True):
    """camera 0: the whole cube; 1 .. 7: the slab that holds about j eighths of it"""
    hi_x = side if j == 0 else (-0.5 + j / 8.0) * side
    v = box_view((-side, -side, -side), (hi_x, side, side))
    v["shadow_pass"] = -1 if main else 0
    v["emit_records"] = int(emitted)
    return v


_REFERENCES = {}


def reference(oracle, key, meshes, sc, view, sort):
    """oracle.prepare_meshes of a copy of the bound pool, cached under `key` (what tells scene, pool, camera and order apart);
    is_visible: the column the oracle wrote (a main pass)"""
    if key not in _REFERENCES:
        pool = meshes.copy()
        exp = oracle.prepare_meshes(pool, sc.transforms, sc.entity_to_transform, view, sort={0: None, 1: "ascending", 2: "descending"}[sort])
        exp["is_visible"] = pool["isVisible"].copy()
        _REFERENCES[key] = exp
        while len(_REFERENCES) > 24:
            _REFERENCES.pop(next(iter(_REFERENCES)))
    return _REFERENCES[key]


def enable_exactly(oracle, sc, meshes, side, k, seed=5):
    """isEnabled on exactly k of the meshes the oracle finds visible under the whole-cube view, cleared on all others"""
    exp = oracle.prepare_meshes(meshes.copy(), sc.transforms, sc.entity_to_transform, camera(0, side))
    chosen = np.random.default_rng(seed + k).choice(exp["visible_idx"], size=k, replace=False)
    meshes["isEnabled"] = 0
    meshes["isEnabled"][chosen] = 1
    return meshes


# ---- delivery and comparison ----

def deliver(vis, pool_id, v, n, layout, emitted):
    """what one gv_pool_results_fetch of (pool, view) hands over, and the record structs behind it"""
    got = vis.fetch(v, write_back=False, occupancy=n, pool_id=pool_id, order="raw")
    if layout is not None and emitted:
        assert got["visible_idx"] is None or got["draw_count"] == 0  # delivered as structs instead
        got["records"] = vis.records(pool_id, v, ds.LAYOUTS[layout][0])
    return got


def records_as_arrays(rec, layout, slot_of=None):
    """(slots, baked_model, distance_sq) of a struct array, after checking what only structs have: every byte no field owns is
    zero, bufferIndex holds the layout's value, componentOffset is a whole multiple of the component size"""
    dt, buffer_index = ds.LAYOUTS[layout]
    assert rec.dtype == dt
    raw = rec.view(np.uint8).reshape(-1, dt.itemsize)
    assert not raw[:, ~ds.covered_bytes(dt)].any(), f"{layout}: a byte no field owns is not zero"
    if buffer_index is not None:
        assert np.all(rec["bufferIndex"] == buffer_index)
    offsets = rec["componentOffset"].astype(np.uint64)
    assert not np.any(offsets % np.uint64(COMPONENT_STRIDE))
    ids = (offsets // np.uint64(COMPONENT_STRIDE)).astype(np.int64)
    slots = ids if slot_of is None else slot_of(ids)
    return slots.astype(np.uint32), np.ascontiguousarray(rec["bakedModel"]), np.ascontiguousarray(rec["distanceSq"])


def assert_delivered(exp, got, n, code, layout, what, slot_of=None):
    assert got["draw_count"] == exp["draw_count"], what
    count = int(exp["draw_count"])
    if code.main:
        assert got["is_visible"] is not None and got["is_visible"].shape == (n,), what
        assert np.array_equal(got["is_visible"], exp["is_visible"]), f"{what}: isVisible differs at slots {np.nonzero(got['is_visible'] != exp['is_visible'])[0][:8]}"
    else:
        assert got["is_visible"] is None, what
    if not code.emitted:
        assert got.get("records") is None and (got["visible_idx"] is None or count == 0), what
        return
    if layout is not None:
        assert got["records"].shape == (count,), what
        slots, model, dist = records_as_arrays(got["records"], layout, slot_of)
    else:
        slots, model, dist = got["visible_idx"], got["baked_model"], got["distance_sq"]
        assert slots is not None and slots.shape == (count,) and model.shape == (count, 12) and dist.shape == (count,), what
    if count == 0:
        return
    if code.sort:
        descending = code.sort == 2
        assert np.all(dist[:-1] >= dist[1:]) if descending else np.all(dist[:-1] <= dist[1:]), what
        o = np.lexsort((slots, -dist if descending else dist))  # ties: canonical by slot
        e = np.arange(count)
    else:
        assert np.unique(slots).shape[0] == count, f"{what}: a slot delivered twice"
        o = np.argsort(slots, kind="stable")
        e = np.argsort(exp["visible_idx"], kind="stable")
    assert np.array_equal(slots[o], exp["visible_idx"][e]), what
    assert np.array_equal(model[o].view(np.uint32), exp["baked_model"][e].view(np.uint32)), what
    assert np.array_equal(dist[o].view(np.uint32), exp["distance_sq"][e].view(np.uint32)), what


def poison(vis, pool_id, v, n, layout, emitted):
    """Overwrites what the library's host buffers hold of a view that has been checked (its fetch here only looks the results up,
    or copies them once more): consecutive frames of a case deliver equal values into the same buffers, and a byte the next
    frame's delivery left out would otherwise pass as the previous frame's.
    Relies on the C-ABI of include/garden_vis.h alone, past the GpuVisibility wrapper (which hands out copies): GvResult's
    is_visible (occupancy bytes), visible_idx / baked_model / distance_sq (draw_count elements of 4 / 48 / 4 bytes) and the
    (records, count) of gv_pool_results_records (count * stride bytes) point into host memory that stays valid and is written
    by nothing until the view's next delivery; a view with a record target gets `leave` instead."""
    import ctypes as C
    from garden_amd.lib import GvResult
    r = GvResult()
    vis._check(vis.lib.gv_pool_results_fetch(vis.ctx, pool_id, v, 0, C.byref(r)))
    if r.is_visible:
        C.memset(r.is_visible, 0x5A, n)
    if r.visible_idx and r.draw_count:
        C.memset(r.visible_idx, 0xEE, 4 * r.draw_count)
        C.memset(r.baked_model, 0xEE, 48 * r.draw_count)
        C.memset(r.distance_sq, 0xEE, 4 * r.draw_count)
    if layout is not None and emitted:
        at, count = C.c_void_p(), C.c_uint32()
        vis._check(vis.lib.gv_pool_results_records(vis.ctx, pool_id, v, C.byref(at), C.byref(count)))
        if at.value and count.value:
            C.memset(at.value, 0xEE, count.value * ds.LAYOUTS[layout][0].itemsize)


def set_layouts(vis, layouts):
    for p, layout in enumerate(layouts):
        if layout is None:
            vis.set_record_layout(p, None)
        else:
            dt, buffer_index = ds.LAYOUTS[layout]
            vis.set_record_layout(p, dt, component_stride=COMPONENT_STRIDE, buffer_index_value=buffer_index or 0)


def run_frame(vis, oracle, key, sc, pools, side, frm, slot_of=None, leave=False):
    """culls and sorts what the frame asks for, fetches in its order, compares every fetched view with the oracle and (unless
    `leave`) poisons the host buffers behind it. Returns {(pool, view): (delivered, expected)}."""
    set_layouts(vis, frm.layouts)
    codes = [ds.parse_views(code) for code in frm.views]
    views = [[camera(c.camera, side, c.main, c.emitted) for c in per_pool] for per_pool in codes]
    for p, per_pool in enumerate(codes):
        vis.cull(p, views[p])
        for v, c in enumerate(per_pool):
            if c.sort:
                vis.sort(v, descending=c.sort == 2, pool_id=p)
    out = {}
    for p, v in ds.fetch_order(frm):
        c, n = codes[p][v], pools[p].shape[0]
        got = deliver(vis, p, v, n, frm.layouts[p], c.emitted)
        exp = reference(oracle, (key, p, n, c.camera, c.main, c.sort), pools[p], sc, views[p][v], c.sort)
        assert_delivered(exp, got, n, c, frm.layouts[p], f"pool {p} ({n} slots, {frm.layouts[p]}) view {v} {frm.views[p].split(',')[v]} fetched {frm.order}",
                         slot_of[p] if slot_of else None)
        out[(p, v)] = (got, exp)
    for p, v in ([] if leave else out):
        poison(vis, p, v, pools[p].shape[0], frm.layouts[p], codes[p][v].emitted)
    return out


def context(keep_slot_order):
    from garden_amd.lib import GpuVisibility
    return GpuVisibility(device=0, keep_slot_order=keep_slot_order)


def bind(vis, sc, pools):
    vis.bind_transforms(sc.transforms, sc.entity_to_transform)
    for p, meshes in enumerate(pools):
        vis.bind_pool(p, meshes)
    vis.hierarchy_rebuild()


def assert_route(route, context_name, n, frm):
    """the model's claim for a one-pool frame: its first fetch takes `route`, every other view that route or `found`"""
    plan = ds.delivery_plan(ds.frame_model(ds.Case("", context_name, (n,), ()), frm))
    assert {cell[0] for cell in plan.values()} <= {route, "found"} and plan[ds.fetch_order(frm)[0]][0] == route


# ---- the cases of the census ----

@pytest.mark.gpu
@pytest.mark.parametrize("c", ds.CASES, ids=lambda c: c.name)
def test_every_delivery_form_matches_the_oracle(oracle, c):
    """the case's frames one after the other in one context: every (pool, view) of every frame equals the oracle, whichever
    fetch delivered it. A pool of the issue's table holds the table's count under the whole-cube view. The pools of 2, 3 and 5
    slots, every slot of which the cube view sees, then have slot 1 disabled: their isVisible column holds a zero among ones,
    so a byte put at the wrong slot shows (a permutation of all ones is all ones)."""
    total = max(c.sizes)
    sc, side = flat(total), scene_side(total)
    pools = [sc.meshes[:n].copy() for n in c.sizes]
    if len(c.sizes) == 1 and total in CUBE_RECORDS:
        exp = reference(oracle, ("table", total), pools[0], sc, camera(0, side), 0)
        assert exp["draw_count"] == CUBE_RECORDS[total]
    if len(c.sizes) == 1 and 2 <= total <= 5:
        pools[0]["isEnabled"][1] = 0
    if len(c.sizes) == 1 and total >= 2:
        column = reference(oracle, (c.sizes, 0, total, 0, True, 0), pools[0], sc, camera(0, side), 0)["is_visible"]
        assert column.any() and not column.all()
    with context(c.context == "slot") as vis:
        bind(vis, sc, pools)
        for frm in c.frames:
            out = run_frame(vis, oracle, c.sizes, sc, pools, side, frm)
            assert len(out) == sum(len(code.split(",")) for code in frm.views)
            if total >= 255:  # not degenerate: some view of the frame holds records (and a main pass drops some slots)
                assert any(exp["draw_count"] > 0 for _got, exp in out.values())


@pytest.mark.gpu
@CONTEXTS
def test_a_sibling_view_is_found_as_the_oracle_has_it(oracle, keep_slot_order):
    """the first fetch of the frame delivers the main pass AND its shadow passes; the siblings' own fetches, in any order, and a
    second fetch of the first view hand out the oracle's results from the host buffers (no further launch of any kind)"""
    n = 5003
    sc, side = flat(n), scene_side(n)
    pools = [sc.meshes.copy()]
    frm = ds.Frm(("wide_128",), ("M,S2,S5,m",), "forward")
    with context(keep_slot_order) as vis:
        bind(vis, sc, pools)
        run_frame(vis, oracle, ("found", n), sc, pools, side, frm, leave=True)
        codes = ds.parse_views(frm.views[0])
        for v in (3, 2, 0, 1, 0):
            got = deliver(vis, 0, v, n, "wide_128", codes[v].emitted)
            exp = reference(oracle, (("found", n), 0, n, codes[v].camera, codes[v].main, 0), pools[0], sc, camera(codes[v].camera, side, codes[v].main), 0)
            assert exp["draw_count"] > 0
            assert_delivered(exp, got, n, codes[v], "wide_128", f"view {v} fetched again")


@pytest.mark.gpu
def test_all_16384_slots_visible_and_sorted_by_the_publishing_sort(oracle):
    """kBatchSortMaxSlots slots, every one visible: the row's last workgroup of the publishing sort both ranks records and
    un-permutes isVisible (a spatially ordered context). The scene's defects are repaired, so the oracle's count is the occupancy."""
    n = ds.BATCH_SORT_MAX
    sc, side = flat(n, defects=False), scene_side(n)
    pools = [sc.meshes.copy()]
    exp = reference(oracle, ("all-visible", 0, n, 0, True, 1), pools[0], sc, camera(0, side), 1)
    assert exp["draw_count"] == n and np.all(exp["is_visible"] == 1)
    with context(False) as vis:
        bind(vis, sc, pools)
        for frm in (ds.Frm(("packed_sorted",), ("Ma",), "forward"), ds.Frm(("wide_128",), ("Ma,Sd",), "reverse")):
            assert ds.delivery_plan(ds.frame_model(ds.Case("", "spatial", (n,), ()), frm))[(0, 0)][0] in ("sort", "found")
            run_frame(vis, oracle, "all-visible", sc, pools, side, frm)


# ---- exact record counts ----

K_SMALL_POOL = 3000
K_EDGES = (0, 1, ds.RECORD_CHUNK - 1, ds.RECORD_CHUNK, ds.RECORD_CHUNK + 1) + tuple(
    ds.publish_grid(K_SMALL_POOL) * ds.RECORD_CHUNK + d for d in (-1, 0, 1))  # the second round of publish_block's chunk loop


@pytest.mark.gpu
@CONTEXTS
@pytest.mark.parametrize("k", K_EDGES)
def test_record_counts_at_the_chunk_and_at_a_round_of_the_publish_grid(oracle, k, keep_slot_order):
    """exactly k records on a 3 000-slot pool (alone in its frame: the publish grid is 12 workgroups, one round of it 768
    records), as structs, as arrays, and through the publishing sort"""
    n = K_SMALL_POOL
    sc, side = flat(n), scene_side(n)
    assert ds.publish_grid(n) * ds.RECORD_CHUNK + 1 <= CUBE_RECORDS[n]
    pools = [enable_exactly(oracle, sc, sc.meshes.copy(), side, k)]
    key = ("k", n, k)
    assert reference(oracle, (key, 0, n, 0, True, 0), pools[0], sc, camera(0, side), 0)["draw_count"] == k
    with context(keep_slot_order) as vis:
        bind(vis, sc, pools)
        for frm in (ds.Frm(("reversed_96",), ("M,S0",), "forward"), ds.Frm((None,), ("M,S0",), "reverse"), ds.Frm(("simd_sorted",), ("Md,Sa0",), "forward")):
            out = run_frame(vis, oracle, key, sc, pools, side, frm)
            assert out[(0, 0)][0]["draw_count"] == k
            if k == 0 and frm.layouts[0]:
                assert all(got["records"].shape == (0,) for got, _exp in out.values())


LARGE_POOL = ds.PUBLISH_MAX + 1


@pytest.mark.gpu
@CONTEXTS
@pytest.mark.parametrize("k", [0, ds.PACK_GRID * ds.RECORD_CHUNK, ds.PACK_GRID * ds.RECORD_CHUNK + 1])
def test_record_counts_at_a_round_of_the_pack_grid(oracle, k, keep_slot_order):
    """the copies route on the 262 145-slot pool, as structs and as arrays (the three copies): 131 072 records are one round of
    pack_records_kernel's 2 048 workgroups, 131 073 begin the second; with none, records() is empty and isVisible all zero"""
    n = LARGE_POOL
    sc, side = flat(n), scene_side(n)
    pools = [enable_exactly(oracle, sc, sc.meshes.copy(), side, k)]
    key = ("k", n, k)
    exp = reference(oracle, (key, 0, n, 0, True, 0), pools[0], sc, camera(0, side), 0)
    assert exp["draw_count"] == k and ds.PACK_GRID * ds.RECORD_CHUNK + 1 <= CUBE_RECORDS[n]
    with context(keep_slot_order) as vis:
        bind(vis, sc, pools)
        for frm in (ds.Frm(("offset4_112",), ("M",), "forward"), ds.Frm((None,), ("M",), "forward"), ds.Frm(("packed",), ("M,S0",), "reverse")):
            assert_route("copies", "slot" if keep_slot_order else "spatial", n, frm)
            got = run_frame(vis, oracle, key, sc, pools, side, frm)[(0, 0)][0]
            assert got["draw_count"] == k
            assert got["records"].shape == (k,) if frm.layouts[0] else got["visible_idx"].shape == (k,)
            if k == 0:
                assert not got["is_visible"].any()


# ---- layouts, on every route ----

ROUTE_POOLS = {"sort": (5003, "Ma,Sd"), "publish": (20_001, "M,S6"), "copies": (LARGE_POOL, "M")}


@pytest.mark.gpu
@CONTEXTS
@pytest.mark.parametrize("route", list(ROUTE_POOLS))
@pytest.mark.parametrize("layout", list(ds.LAYOUTS))
def test_every_layout_on_every_route(oracle, layout, route, keep_slot_order):
    """64 to 128 bytes, fields in and out of declaration order, componentOffset at a 4- but not 8-aligned offset, bufferIndex
    in the last word with its top bit set: every field where the layout puts it, every other byte zero, and componentOffset
    = slot * 2^20 in all 64 bits (some delivered record lies beyond 2^32)"""
    n, views = ROUTE_POOLS[route]
    sc, side = flat(n), scene_side(n)
    pools = [sc.meshes.copy()]
    frm = ds.Frm((layout,), (views,), "forward")
    assert_route(route, "slot" if keep_slot_order else "spatial", n, frm)
    with context(keep_slot_order) as vis:
        bind(vis, sc, pools)
        out = run_frame(vis, oracle, ("layouts", n), sc, pools, side, frm)
        for got, exp in out.values():
            assert exp["draw_count"] > 0
            assert int(got["records"]["componentOffset"].max()) >= 1 << 32 and int(exp["visible_idx"].max()) >= 4096


@pytest.mark.gpu
@CONTEXTS
@pytest.mark.parametrize("route", list(ROUTE_POOLS))
def test_records_in_world_slots_on_every_route(oracle, route, keep_slot_order):
    """GV_RESULTS_MAP_RECORDS with a non-monotone index map whose ids lie well above the occupancy:
    componentOffset == map[slot] * component size; everything else as without the map"""
    from garden_amd.lib import GV_RESULTS_MAP_RECORDS
    n, views = ROUTE_POOLS[route]
    sc, side = flat(n), scene_side(n)
    pools = [sc.meshes.copy()]
    ids = (np.random.default_rng(n).permutation(n).astype(np.uint32) * np.uint32(5) + np.uint32(10 * n + 7))
    assert ids.min() > 4 * n and np.any(np.diff(ids.astype(np.int64)) < 0) and np.unique(ids).shape[0] == n
    back = np.full(int(ids.max()) + 1, -1, np.int64)
    back[ids] = np.arange(n)

    def slot_of(got_ids):
        assert got_ids.max(initial=0) < back.shape[0] and np.all(back[got_ids] >= 0), "a componentOffset that is no id of the map"
        return back[got_ids]

    frm = ds.Frm(("reversed_96",), (views,), "forward")
    assert_route(route, "slot" if keep_slot_order else "spatial", n, frm)
    with context(keep_slot_order) as vis:
        bind(vis, sc, pools)
        vis.set_index_map(0, ids)
        vis.set_result_mapping(0, GV_RESULTS_MAP_RECORDS)
        out = run_frame(vis, oracle, ("layouts", n), sc, pools, side, frm, slot_of=[slot_of])
        for got, exp in out.values():
            assert exp["draw_count"] > 0
            assert np.array_equal(np.sort(got["records"]["componentOffset"]), np.sort(ids[exp["visible_idx"]].astype(np.uint64) * np.uint64(COMPONENT_STRIDE)))


# ---- record targets ----

@pytest.mark.gpu
@CONTEXTS
@pytest.mark.parametrize("route", list(ROUTE_POOLS))
def test_a_record_target_receives_exactly_the_records_on_every_route(oracle, route, keep_slot_order):
    """the caller's array, pre-filled with 0xAB: bytes [0, count * stride) equal records() — which equal the oracle —, everything
    behind is untouched. The publish and the copies case stage more than 1 MB, no multiple of 256 KB: the staged copy runs in
    pieces over the worker threads."""
    n, views = ROUTE_POOLS[route]
    sc, side = flat(n), scene_side(n)
    pools = [sc.meshes.copy()]
    dt = ds.LAYOUTS["packed"][0] if route != "sort" else ds.LAYOUTS["wide_128"][0]
    layout = "packed" if route != "sort" else "wide_128"
    codes = ds.parse_views(views)
    frm = ds.Frm((layout,), (views,), "forward")
    assert_route(route, "slot" if keep_slot_order else "spatial", n, frm)
    targets = [np.full(n * dt.itemsize, 0xAB, np.uint8) for _ in codes]
    with context(keep_slot_order) as vis:
        bind(vis, sc, pools)
        for v, target in enumerate(targets):
            vis.set_record_target(0, v, target)
        for _tick in range(2):  # the same arrays every frame, as an engine's vectors are
            out = run_frame(vis, oracle, ("layouts", n), sc, pools, side, frm, leave=True)  # (the targets are poisoned below)
            for v, target in enumerate(targets):
                got, exp = out[(0, v)]
                count = int(exp["draw_count"])
                staged = count * dt.itemsize
                assert count > 0 and np.array_equal(target[:staged], got["records"].view(np.uint8))
                assert np.all(target[staged:] == 0xAB), "bytes behind the records were written"
                if route != "sort" and v == 0:
                    assert staged >= 1 << 20 and staged % (256 << 10) != 0
                target[:staged] = 0xAB
        for v in range(len(targets)):
            vis.set_record_target(0, v, None)
