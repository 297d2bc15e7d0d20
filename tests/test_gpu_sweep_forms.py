"""GPU parity of the world-matrix chain (calc_model -> mul_affine / mfma_chain_step -> model_rows) in every form that runs it —
gv_sweep VALU, MFMA, the two sweeps fused with a cull, the incremental subtree sweep — and in its consumers (cull, emit, batched
cull, sphere stream), on the worlds of tests/sweep_support.py: tile and wave edges of the sweep stages with chains placed lane
by lane, numeric extremes (subnormals, underflow, overflow, -0, zero and non-unit quaternions, huge scales, NaN born inside the
chain), 300-link chains, and a sphere stream whose radii are subnormal, overflow or are not finite.

The contract checked is DESIGN.md §2's: world matrices, bakedModel and distanceSq equal the oracle's bit for bit for finite values,
subnormals, +-0 and +-inf, and are NaN where the oracle's are NaN (same_floats); visible sets, draw counts and isVisible bytes
are exact. tests/test_sweep_census.py proves on the CPU that the worlds hold these classes and that NaN rows stay a minority.
The GPU forms are also compared with each other, bitwise outside the oracle's NaN positions; the number of NaN elements whose
bit patterns differ between two forms is printed, not asserted (DESIGN.md §2 records the observed figure)."""
import numpy as np
import pytest

import cull_paths_support as cp
import sweep_support as ss
from garden_amd import scene
from garden_amd.lib import (GV_DIRTY_HIERARCHY, GV_DIRTY_TRANSFORM, GV_SWEEP_INCREMENTAL, GV_SWEEP_MFMA, GV_SWEEP_VALU,
                            GV_SWEEP_WITH_CULL, GV_SWEEP_WITH_CULL_VALU)

pytestmark = pytest.mark.gpu

COUNTED = ("cull", "scan", "emit", "sweep")  # the launch counters of GvStats a cull plan speaks of (tests/test_gpu_cull_paths.py)
_PYRAMIDS = {}


def pyramid(oracle, size=(256, 128)):
    """(depth image, the oracle's pyramid of it), built once per size"""
    if size not in _PYRAMIDS:
        depth = scene.synthetic_depth(*size, rects=12)
        depth.setflags(write=False)
        _PYRAMIDS[size] = (depth, oracle.Hiz(depth))
    return _PYRAMIDS[size]


def bind(vis, oracle, sc, size=(256, 128)):
    depth, hz = pyramid(oracle, size)
    vis.bind_transforms(sc.transforms, sc.entity_to_transform)
    vis.bind_pool(0, sc.meshes)
    vis.hierarchy_rebuild()
    vis.hiz_build(depth)
    return hz


def assert_same(got, exp, what):
    bad = ss.same_floats(got, exp)
    if bad.size:
        g, e = np.ravel(got).view(np.uint32)[bad[:6]], np.ravel(exp).view(np.uint32)[bad[:6]]
        width = got.shape[-1] if got.ndim > 1 else 1
        raise AssertionError(f"{what}: {bad.size} elements differ; (row, column): got / expected bits " +
                             ", ".join(f"({i // width}, {i % width}): {a:08x} / {b:08x}" for i, a, b in zip(bad[:6], g, e)))


def check_cull(vis, oracle, sc, views, hz, what):
    """one gv_cull of `views` against the oracle; returns the launch counters as they stood right behind the cull"""
    vis.cull(0, views)
    launches = vis.stats()["launches"]
    for vi, v in enumerate(views):
        got = vis.fetch(vi, write_back=False, occupancy=sc.count)
        m2 = sc.meshes.copy()
        exp = oracle.prepare_meshes(m2, sc.transforms, sc.entity_to_transform, v, hiz=hz if v.get("use_hiz") else None)
        assert got["draw_count"] == exp["draw_count"], (what, vi, got["draw_count"], exp["draw_count"])
        o = np.argsort(exp["visible_idx"], kind="stable")
        assert np.array_equal(got["visible_idx"], exp["visible_idx"][o]), (what, vi)
        assert_same(got["baked_model"], exp["baked_model"][o], f"{what} view {vi} bakedModel")
        assert_same(got["distance_sq"], exp["distance_sq"][o], f"{what} view {vi} distanceSq")
        if v["shadow_pass"] < 0:
            assert np.array_equal(got["is_visible"], m2["isVisible"]), (what, vi)
    return launches


def world_of(vis, oracle, sc, what):
    """the whole world-matrix cache, checked against the oracle's; returns (cache, oracle's)"""
    exp = oracle.world_matrices(sc.transforms, sc.entity_to_transform)
    got = vis.get_world(0, sc.transforms.shape[0])
    assert_same(got, exp, f"{what} world matrices")
    return got, exp


def scrub(vis, sc, view, mode):
    """Every form under test writes into a cache, result buffers and isVisible bytes that the form before it left holding the
    very values expected of it: a store it skipped would go unseen. So in front of each form the same pools are swept (by
    ANOTHER form: `mode`) and culled in a state in which every live slot has another world matrix, and then put back."""
    tr, nt = sc.transforms, sc.transforms.shape[0]
    saved = tr.copy()
    tr["position"][:, :3] = (12345.0 + np.arange(nt, dtype=np.float32))[:, None]
    tr["scale"][:, :3] = np.float32(1.0)  # (translations only: a 300-link chain stays finite)
    tr["rotation"] = (0, 0, 0, 1)
    vis.mark_dirty(GV_DIRTY_TRANSFORM, 0, nt)
    vis.sweep(mode)
    vis.cull(0, [view])
    vis.wait()
    tr[:] = saved
    vis.mark_dirty(GV_DIRTY_TRANSFORM, 0, nt)


def sweep_forms(vis, oracle, sc, view, hz, what, fused=True):
    """All four full sweep forms over the bound world, the fused ones under one single-view cull each with and without Hi-Z,
    each behind a scrub(); returns {form: world matrices}. fused: the pool is exactly paired, so GV_SWEEP_WITH_CULL[_VALU] must
    ride on the cull's launch (no sweep launch of its own); otherwise the plan falls back to one sweep launch in front of the cull."""
    worlds = {}
    for name, mode in (("valu", GV_SWEEP_VALU), ("mfma", GV_SWEEP_MFMA)):
        scrub(vis, sc, view, GV_SWEEP_MFMA if mode == GV_SWEEP_VALU else GV_SWEEP_VALU)
        vis.stats_reset()
        vis.sweep(mode)
        assert vis.stats()["launches"]["sweep"] == 1, (what, name)
        worlds[name], _ = world_of(vis, oracle, sc, f"{what} sweep({name})")
    for name, mode in (("fused_mfma", GV_SWEEP_WITH_CULL), ("fused_valu", GV_SWEEP_WITH_CULL_VALU)):
        for use_hiz in (0, 1):
            form = name + ("_hiz" if use_hiz else "")
            scrub(vis, sc, dict(view, use_hiz=use_hiz), GV_SWEEP_VALU)
            vis.sweep(mode)
            vis.stats_reset()
            launches = check_cull(vis, oracle, sc, [dict(view, use_hiz=use_hiz)], hz, f"{what} {form}")
            assert launches["cull"] == 1 and launches["sweep"] == (0 if fused else 1), (what, form, launches)
            worlds[form], _ = world_of(vis, oracle, sc, f"{what} {form}")
    return worlds


def forms_agree(worlds, exp, what):
    """form against form: bitwise outside the oracle's NaN positions; the NaN elements whose patterns differ are counted only"""
    nan = np.isnan(exp)
    names = list(worlds)
    first = worlds[names[0]].view(np.uint32)
    differing = 0
    for name in names[1:]:
        other = worlds[name].view(np.uint32)
        assert np.array_equal(first[~nan], other[~nan]), f"{what}: {names[0]} and {name} differ outside the NaN positions"
        differing += int(np.count_nonzero(first[nan] != other[nan]))
    patterns = sorted({f"{int(b):08x}" for w in worlds.values() for b in np.unique(w.view(np.uint32)[nan])})
    from_oracle = int(np.count_nonzero(first[nan] != exp.view(np.uint32)[nan]))
    print(f"NaN patterns, {what}: {int(nan.sum())} NaN elements, {differing} differ between {names[0]} and another of {len(names)} forms, "
          f"{from_oracle} between {names[0]} and the oracle; patterns {patterns}")
    return differing


def incremental_after(vis, oracle, sc, slots, what):
    """`slots` were edited and marked: GV_SWEEP_INCREMENTAL launches once and leaves the oracle's cache; a full VALU sweep agrees"""
    before = vis.stats()["launches"]["sweep"]
    vis.sweep(GV_SWEEP_INCREMENTAL)
    assert vis.stats()["launches"]["sweep"] == before + 1, what
    inc, exp = world_of(vis, oracle, sc, f"{what} incremental")
    vis.sweep(GV_SWEEP_VALU)
    full, _ = world_of(vis, oracle, sc, f"{what} full sweep behind the incremental one")
    forms_agree(dict(incremental=inc, valu=full), exp, f"{what} incremental")


# ---- 1. tile and wave edges ----
TILE_CASES = ([("gpu_slot_order", n, n) for n in ss.TILE_COUNTS] + [("gpu_slot_order", nt, nm) for nt, nm in ss.TILE_MESH_ENDS] +
              [("gpu_slot_order",) + ss.TILE_UNPAIRED] + [("gpu", n, n) for n in (65, 257, 513)])


@pytest.mark.parametrize("ctx_name,nt,nm", TILE_CASES, ids=lambda x: str(x))
def test_tile_edges_every_form(request, oracle, ctx_name, nt, nm):
    """Pools that end on, one before and one past every wave (64), wave stage (192 float4), workgroup (256) and workgroup stage
    (768 float4) boundary; waves of roots only (the fused MFMA form's shortcut), waves with one chained lane (63, 0), depths 0..7
    lane by lane, parents in other workgroups; mesh pools that end before the transform pool (lanes, waves and workgroups that
    only sweep) and one that is longer (not paired: the sweep takes a launch of its own). In the spatial context gv_get_world's
    pool-slot gather takes part."""
    vis = request.getfixturevalue(ctx_name)
    sc = ss.tile_world(nt, nm, 0)
    hz = bind(vis, oracle, sc)
    assert vis.stats()["max_depth"] == (7 if nt > 199 else (1 if nt > 127 else 0))
    what = f"tile_world({nt}, {nm}) {ctx_name}"
    worlds = sweep_forms(vis, oracle, sc, ss.tile_view(), hz, what, fused=nm <= nt)
    exp = oracle.world_matrices(sc.transforms, sc.entity_to_transform)
    assert not np.isnan(exp).any()
    assert forms_agree(worlds, exp, what) == 0


# ---- 2. numeric extremes ----
@pytest.mark.parametrize("ctx_name", ["gpu", "gpu_slot_order", "gpu_bounds"])
@pytest.mark.parametrize("n,seed", ss.EDGE_WORLDS)
def test_numeric_extremes_every_form_and_consumer(request, oracle, ctx_name, n, seed):
    vis = request.getfixturevalue(ctx_name)
    sc = ss.edge_world(n, seed)
    hz = bind(vis, oracle, sc)
    what = f"edge_world({n}, {seed}) {ctx_name}"
    views = ss.edge_views()
    worlds = sweep_forms(vis, oracle, sc, views[0][1], hz, what)
    forms_agree(worlds, oracle.world_matrices(sc.transforms, sc.entity_to_transform), what)
    # plain cull + fetch (no sort): records from the resident cache, then — every transform re-mirrored — from the chain itself
    for cache in ("resident", "stale"):
        if cache == "stale":
            vis.mark_dirty(GV_DIRTY_TRANSFORM, 0, n)
        for name, view in views:
            for use_hiz in (0, 1):
                check_cull(vis, oracle, sc, [dict(view, use_hiz=use_hiz)], hz, f"{what} {name} hiz={use_hiz} cache {cache}")
    batch = ss.edge_batch()
    check_cull(vis, oracle, sc, batch, hz, f"{what} batched")
    check_cull(vis, oracle, sc, [dict(batch[0], use_hiz=1)] + batch[1:], hz, f"{what} batched behind Hi-Z")
    # the incremental form: fresh extremes, one of each class, into scattered slots (half of them interior nodes)
    vis.sweep(GV_SWEEP_VALU)
    rng = np.random.Generator(np.random.PCG64(n + seed))
    live = np.flatnonzero(sc.transforms["entity"] != 0)
    inner = np.intersect1d(ss.interior_slots(sc), live)
    slots = np.unique(np.concatenate([rng.choice(inner, 6, replace=False), rng.choice(live, 6, replace=False)]))
    ss.replant(sc, slots, rng)
    for s in slots:
        vis.mark_dirty(GV_DIRTY_TRANSFORM, int(s), 1)
    incremental_after(vis, oracle, sc, slots, what)
    check_cull(vis, oracle, sc, [views[0][1]], hz, f"{what} after the edits")


# ---- 3. deep chains ----
@pytest.mark.parametrize("ctx_name", ["gpu", "gpu_slot_order"])
@pytest.mark.parametrize("scale", ss.DEEP_SCALES)
def test_deep_chains(request, oracle, ctx_name, scale):
    """A 300-link chain: the bound of the MFMA loop, chain_model and the subtree walk (max_depth = 299), the product walking down
    through the subnormal range to zero (0.6), up to inf and NaN (1.6), or staying put (1.0). Then the chain is cut in two."""
    vis = request.getfixturevalue(ctx_name)
    sc = ss.deep_world(ss.DEEP_LENGTH, scale)
    hz = bind(vis, oracle, sc)
    assert vis.stats()["max_depth"] == ss.DEEP_LENGTH - 1
    what = f"deep_world({ss.DEEP_LENGTH}, {scale}) {ctx_name}"
    view = ss.deep_view(scale)
    worlds = sweep_forms(vis, oracle, sc, view, hz, what)
    forms_agree(worlds, oracle.world_matrices(sc.transforms, sc.entity_to_transform), what)
    check_cull(vis, oracle, sc, [view], hz, f"{what} cull")
    check_cull(vis, oracle, sc, [dict(view, use_hiz=1)], hz, f"{what} cull behind Hi-Z")
    vis.sweep(GV_SWEEP_VALU)
    sc.transforms["parent"][150] = sc.transforms["entity"][0]
    vis.mark_dirty(GV_DIRTY_HIERARCHY, 150, 1)
    sc.transforms["position"][1, :3] += np.float32(0.5)
    vis.mark_dirty(GV_DIRTY_TRANSFORM, 1, 1)
    incremental_after(vis, oracle, sc, [1, 150], f"{what} re-parented")
    assert vis.stats()["max_depth"] == 150
    check_cull(vis, oracle, sc, [view], hz, f"{what} cull after the re-parenting")


# ---- 4. the sphere stream ----
def test_sphere_stream_with_extremes(gpu_linear, oracle):
    """cull_hot_kernel decides from (position, sphere_radius) stored once per entry: radii that are subnormal, that overflow to inf
    from finite inputs or are NaN, a reach whose magnitude overflows, boxes of extent 1e-42 and 3e18, positions +-3e38. The
    launch counters must be those of the sphere-stream plan (its build on the first cull, its patch after 30 itemised edits)."""
    vis = gpu_linear
    sc = ss.sphere_world()
    n = ss.SPHERE_N
    hz = bind(vis, oracle, sc, size=(1024, 512))
    flags = cp.FIXTURE_FLAGS["gpu_linear"]
    # a known state, as tests/test_gpu_cull_paths.py brings it about: two quiet culls, then every transform re-mirrored
    settle = cp.make_views("C", 99, cp.scene_side(n))
    vis.cull(0, settle)
    vis.cull(0, settle)
    vis.mark_dirty(GV_DIRTY_TRANSFORM, 0, n)
    state = cp.PoolModel()
    state.seen_at = state.stamp
    state.edit(n, n)
    upkeep = []

    def cull(view, what):
        plan = cp.cull_plan(n, n, "exact", 0, [cp.View(True, bool(view.get("use_hiz")), True)], flags, state=state)
        assert plan.cull_form == "plain_hot", what
        vis.stats_reset()
        launches = check_cull(vis, oracle, sc, [view], hz, f"sphere_world {what}")
        assert {k: launches[k] for k in COUNTED} == plan.launches, (what, launches, plan.launches, plan.upkeep)
        upkeep.extend(plan.upkeep)

    views = ss.sphere_views()
    for name, view in views:
        cull(view, name)
    cull(dict(views[0][1], use_hiz=1), "perspective behind Hi-Z")
    assert upkeep == ["hot_build"]
    rng = np.random.Generator(np.random.PCG64(30))
    slots = np.sort(rng.choice(np.flatnonzero(sc.planted & (sc.transforms["entity"] != 0)), 30, replace=False))
    ss.replant(sc, slots, rng)
    for s in slots:
        vis.mark_dirty(GV_DIRTY_TRANSFORM, int(s), 1)
    state.edit(n, 30)
    for name, view in views:
        cull(view, f"{name} after 30 edits")
    cull(dict(views[0][1], use_hiz=1), "perspective behind Hi-Z after 30 edits")
    assert upkeep == ["hot_build", "hot_patch"]
